-- objective_hip.lua -- drop-in for the reference's objective.lua on libfrcnn_hip.so: the same two globals
-- (extract_roi_pooling_input, create_objective) with the same arguments and results, same per-image structure as
-- objective.lua:45-218 (pnet forward, sparse RPN loss on the sampled anchors, ROI adaptive max-pooling, cnet
-- forward/backward, ROI-pool backward, pnet backward; normalise; log) -- but every per-example Lua loop that touched
-- the device one scalar at a time is ONE batched call (frcnn_pnet_anchor_loss_begin, frcnn_roi_pool_forward/backward,
-- frcnn_cnet_losses), and the statistics of objective.lua:52-58 stay in a device-side fp64 vector until the single
-- read-back at the end.  1:1 with the tested Python host mirror (faster-rcnn.torch_amd/objective.py); this image has no
-- Lua runtime, so this file is checked statically (tests/test_abi.py) and has not been executed.
--
--   main.lua:  require 'objective'  ->  require 'objective_hip'
local ffi = require 'ffi'
local hip = require 'frcnn_hip'
require 'Localizer'          -- the reference's own files, unchanged
require 'Anchors'
local C, check = hip.C, hip.check

-- objective.lua:5-13.  The strided view `feature_layer_output[idx]` is never materialised: the batched ROI-pooling
-- kernel reads the window in place, so the first result is the index table as well.
function extract_roi_pooling_input(input_rect, localizer, feature_layer_output)
  local r = localizer:inputToFeatureRect(input_rect)
  local s = feature_layer_output:size()
  r = r:clip(Rect.new(0, 0, s[3], s[2]))
  local idx = { {}, { math.min(r.minY + 1, r.maxY), r.maxY }, { math.min(r.minX + 1, r.maxX), r.maxX } }
  return idx, idx
end

function create_objective(model, weights, gradient, batch_iterator, stats)
  local cfg = model.cfg
  local pnet = model.pnet
  local cnet = model.cnet
  local native = model.native

  local bgclass = cfg.class_count + 1                                   -- :20
  local nheads = #model.anchor_nets
  local localizer = Localizer.new(pnet.outnode.children[nheads + 1])   -- :22 (children[5])
  local kh, kw, method, sampling = hip.roi_pooling_settings(cfg)
  local align = method == 'align'                    -- RoIAlign: the double rects themselves in the place of the snapped windows
  local inv_sx, inv_sy = 0, 0
  if align then inv_sx, inv_sy = hip.align_geometry(localizer) end
  local cnet_input_planes = model.layers[#model.layers].filters
  local D = kh * kw * cnet_input_planes
  local ncls = cfg.class_count + 1
  local acc = hip.buffer(8 * 8)        -- {cls_loss, reg_loss, -, -, creg_loss, ccls_loss, -, -} as device doubles
  local acc_host = ffi.new('double[8]')
  local scratch = hip.scratch()
  -- cfg.roi_sampling (INTEGRATION.md): under source = 'proposals' the classification net's rows are a sample of the first NMS's
  -- candidates on the pass's own head maps (hip.sample_proposals: scan, selection, NMS, frcnn_proposal_targets_batch); under
  -- source = 'hard' every labelled candidate is pooled and scored in evaluate mode first, and the rows of largest loss train
  -- (hip.mine_hard: frcnn_roi_hard_keys_batch, the NMS keyed by the loss, frcnn_roi_hard_gather_batch)
  local rs_state = { images = 0 }
  local keep_gt
  local keep                            -- host staging of the last example tables (must outlive the queued copy)

  local function cleanAnchors(examples, outputs)                        -- :32-43
    local i = 1
    while i <= #examples do
      local anchor = examples[i][1]
      local fmSize = outputs[anchor.layer]:size()
      if anchor.index[2] > fmSize[2] or anchor.index[3] > fmSize[3] then
        table.remove(examples, i)
      else
        i = i + 1
      end
    end
  end

  -- staged training (cfg.train, read at every call; INTEGRATION.md): the settings as they stand, validated
  local nblocks = #model.layers
  local function stage()
    local fb, proposal, classification = hip.train_settings(model.cfg, nblocks)
    return fb, proposal, classification, hip.trainable_ranges(model, fb, proposal, classification)
  end
  -- the optim overrides (frcnn_hip.lua) update the slices published here, keyed by the weight tensor
  -- ... and fill stats.gnorm / stats.skipped when config.clipNorm / config.skipNonFinite turn the gradient guard on
  local published = { ranges = function() return select(4, stage()) end, stats = stats }
  hip.trainable[weights] = published

  local function lossAndGradient(w)
    -- before anything is queued: a bad cfg.train raises here.  The library skips the frozen parts' work, this pass skips a
    -- disabled stage, the optimiser updates `ranges` only
    local frozen_blocks, proposal, classification, ranges = stage()
    local rs = hip.roi_sampling_settings(cfg)         -- (validated, like cfg.train, before anything is queued)
    -- cfg.cnet_loss (INTEGRATION.md): nil -- the reference's losses (frcnn_cnet_losses) -- or the description of
    -- frcnn_cnet_loss_rows, whose rows frcnn_loss_accumulate sums into the same two accumulators
    local cl = hip.cnet_loss_settings(cfg)
    local cl_desc = cl and hip.cnet_loss_desc(cl, bgclass) or nil
    if rs and ((rs.source ~= 'proposals' and rs.source ~= 'hard') or not classification) then rs = nil end
    check(C.frcnn_model_set_trainable(native, frozen_blocks, proposal and 1 or 0, classification and 1 or 0))
    published.pass = ranges
    if w ~= weights then weights:copy(w) end                            -- :46-48
    gradient:zero()                                                     -- :49
    check(C.frcnn_zero(acc.ptr, 64, nil))
    local cls_count, reg_count = 0, 0                                   -- :52-58 (the four losses live in `acc`)
    local creg_count, ccls_count = 0, 0
    pnet:training()                                                     -- :61-62
    cnet:training()

    local batch = batch_iterator:nextTraining()                         -- :64
    for _, x in ipairs(batch) do
      local img = hip.to_device(x.img)                                  -- :66
      local p, n = x.positive, x.negative
      -- :71 (anchor nets stay in flight; sampled proposals: the scan reads their dense maps on this stream, so the pass waits)
      local outputs = pnet:forward(img, rs == nil)
      cleanAnchors(p, outputs)                                          -- :74-75
      cleanAnchors(n, outputs)
      local delta_outputs = pnet:delta_outputs()                        -- :78-84
      local npos, nneg = #p, #n
      local E = npos + nneg
      local fm = outputs[nheads + 1]
      local fs = fm:size()

      local F_rows = npos
      local d_gt, d_gc, G
      if rs then                                      -- the ground truth of the proposal-target layer, uploaded on this stream
        local gt, gcls
        gt, gcls, G = hip.ground_truth_table(x, cfg.class_count)
        keep_gt = { gt, gcls }
        local g1 = math.max(G, 1)
        local dg = scratch('rs_gt', 36 * g1).ptr
        check(C.frcnn_memcpy_h2d(dg, gt, 32 * g1, nil))
        check(C.frcnn_memcpy_h2d(dg + 32 * g1, gcls, 4 * g1, nil))
        d_gt, d_gc = ffi.cast('const double*', dg), ffi.cast('const int*', dg + 32 * g1)
      end

      if E > 0 then
        -- ---- host: the example tables, one upload ----------------------------------------------
        local np1 = math.max(npos, 1)
        local ex_anchor = ffi.new('double[?]', 4 * E)
        local ex_roi = ffi.new('double[?]', 4 * np1)
        local ex_idx = ffi.new('int[?]', 4 * E)
        local ex_class = ffi.new('int[?]', np1)
        local wins = ffi.new(align and 'double[?]' or 'int[?]', 4 * E)
        local seen, sp = {}, {}
        for l = 1, nheads do seen[l] = {}; sp[l] = {} end
        for i = 1, E do
          local a = (i <= npos) and p[i][1] or n[i - npos][1]
          local o = 4 * (i - 1)
          ex_anchor[o], ex_anchor[o + 1], ex_anchor[o + 2], ex_anchor[o + 3] = a.minX, a.minY, a.maxX, a.maxY
          ex_idx[o], ex_idx[o + 1], ex_idx[o + 2], ex_idx[o + 3] = a.layer, a.aspect, a.index[2], a.index[3]
          local pooled = a                                              -- negatives pool the anchor rect itself (:137)
          if i <= npos then
            local roi = p[i][2]
            if roi.class_index < 1 or roi.class_index > cfg.class_count then
              error(string.format('roi.class_index %d outside 1..%d', roi.class_index, cfg.class_count))
            end
            ex_roi[o], ex_roi[o + 1], ex_roi[o + 2], ex_roi[o + 3] = roi.rect.minX, roi.rect.minY, roi.rect.maxX, roi.rect.maxY
            ex_class[i - 1] = roi.class_index
            pooled = roi.rect                                           -- positives pool the ground-truth rect (:117)
          end
          if align then
            wins[o], wins[o + 1], wins[o + 2], wins[o + 3] = pooled.minX, pooled.minY, pooled.maxX, pooled.maxY
          else
            local _, idx = extract_roi_pooling_input(pooled, localizer, fm)
            wins[o], wins[o + 1], wins[o + 2], wins[o + 3] = idx[2][1], idx[2][2], idx[3][1], idx[3][2]
          end
          -- where delta_outputs[l] will be non-zero (hint for the sparse anchor-net backward)
          local pos = (a.index[2] - 1) * outputs[a.layer]:size(3) + (a.index[3] - 1)
          if not seen[a.layer][pos] then
            seen[a.layer][pos] = true
            table.insert(sp[a.layer], pos)
          end
        end
        local nsp = 0
        for l = 1, nheads do table.sort(sp[l]); nsp = nsp + #sp[l] end
        local sp_all = ffi.new('int[?]', math.max(nsp, 1))
        local k = 0
        for l = 1, nheads do
          for _, v in ipairs(sp[l]) do sp_all[k] = v; k = k + 1 end
        end
        local b_anchor, b_roi, b_idx, b_class, b_wins, b_sp = 32 * E, 32 * np1, 16 * E, 4 * np1, (align and 32 or 16) * E, 4 * nsp
        local pad = align and (-(b_anchor + b_roi + b_idx + b_class)) % 8 or 0      -- (the rects are doubles: 8-byte offset)
        local total = b_anchor + b_roi + b_idx + b_class + pad + b_wins + b_sp
        local blob = ffi.new('uint8_t[?]', total)
        local o = 0
        ffi.copy(blob + o, ex_anchor, b_anchor); local o_anchor = o; o = o + b_anchor
        ffi.copy(blob + o, ex_roi, b_roi); local o_roi = o; o = o + b_roi
        ffi.copy(blob + o, ex_idx, b_idx); local o_idx = o; o = o + b_idx
        ffi.copy(blob + o, ex_class, b_class); local o_class = o; o = o + b_class + pad
        ffi.copy(blob + o, wins, b_wins); local o_wins = o; o = o + b_wins
        if nsp > 0 then ffi.copy(blob + o, sp_all, b_sp) end
        local o_sp = o
        keep = blob
        local dblob = scratch('blob', total).ptr
        check(C.frcnn_memcpy_h2d(dblob, blob, total, nil))
        for l = 1, nheads do
          check(C.frcnn_pnet_set_sparse_deltas(native, l, ffi.cast('const int*', dblob + o_sp), #sp[l]))
          o_sp = o_sp + 4 * #sp[l]
        end

        -- ---- RPN loss on the sampled anchors (:91-140), queued behind the anchor nets on the library's side
        -- stream and followed by their backward pass; this stream goes on with the last map -------------------
        local ex_loss = ffi.cast('double*', scratch('ex_loss', 16 * E).ptr)
        local crtarget = ffi.cast('float*', scratch('crtarget', 16 * E).ptr)
        local cctarget = ffi.cast('float*', scratch('cctarget', 4 * E).ptr)
        check(C.frcnn_pnet_anchor_loss_begin(native, weights.ptr, gradient.ptr, ffi.cast('const int*', dblob + o_idx),
                                             ffi.cast('const double*', dblob + o_anchor), ffi.cast('const double*', dblob + o_roi),
                                             ffi.cast('const int*', dblob + o_class), npos, nneg, bgclass, ex_loss, crtarget,
                                             cctarget, ffi.cast('double*', acc.ptr), nil))
        if rs then
          -- (the sampled-proposals stage below takes the place of the example rows)
        elseif not classification then
          -- staged training without the detector stage: no ROI pooling, no cnet (dcls / dreg are NaN below); its dropout
          -- stream advances as its forward would advance it
          cnet.seed = (cnet.seed or 0) + 1
          check(C.frcnn_pnet_anchor_loss_wait(native, nil))             -- (the accumulators are read on this stream)
        else
        -- ---- ROI pooling of every example in one launch (:117-119, :137-139) ---------------------------------
        local cinput = hip.view(scratch('cinput', 4 * E * D).ptr, { E, D })
        local pidx
        if align then
          check(C.frcnn_roi_align_forward(fm.ptr, fs[1], fs[2], fs[3], ffi.cast('const double*', dblob + o_wins), nil, E, inv_sx,
                                          inv_sy, kh, kw, sampling, cinput.ptr, nil))
        else
          pidx = ffi.cast('int*', scratch('pidx', 4 * E * D).ptr)
          check(C.frcnn_roi_pool_forward(fm.ptr, fs[1], fs[2], fs[3], ffi.cast('const int*', dblob + o_wins), E, kh, kw,
                                         cinput.ptr, pidx, nil))
        end
        -- ---- fine-tuning stage (:146-186) --------------------------------------------------------------------
        -- (a per-class box head, cfg.box_head, reads the classes of the example table: final on this stream since the upload)
        local coutputs = cnet:forward(cinput, model.box_per_class and { 'int', ffi.cast('const int*', dblob + o_class), npos } or nil)  -- :164
        local crout, ccout = coutputs[1], coutputs[2]
        local crdelta = hip.view(scratch('crdelta', 16 * E).ptr, { E, 4 })
        local ccdelta = hip.view(scratch('ccdelta', 4 * E * ncls).ptr, { E, ncls })
        check(C.frcnn_pnet_anchor_loss_wait(native, nil))               -- crtarget is relative to the proposals (:156)
        if cl_desc == nil then
          check(C.frcnn_cnet_losses(crout.ptr, crtarget, ccout.ptr, cctarget, E, npos, ncls, crdelta.ptr, ccdelta.ptr,
                                    ffi.cast('double*', acc.ptr) + 4, nil))               -- :170-177
        else
          hip.cnet_losses(cl_desc, scratch, crout.ptr, crtarget, ccout.ptr, cctarget, E, npos, ncls, crdelta.ptr, ccdelta.ptr,
                          ffi.cast('double*', acc.ptr) + 4)
        end
        local post_roi_delta = cnet:backward(cinput, { crdelta, ccdelta })              -- :179
        if frozen_blocks < nblocks and align then       -- (a frozen backbone: the library left the input gradient unwritten)
          check(C.frcnn_roi_align_backward(delta_outputs[nheads + 1].ptr, fs[1], fs[2], fs[3], post_roi_delta.ptr,
                                           ffi.cast('const double*', dblob + o_wins), nil, E, inv_sx, inv_sy, kh, kw, sampling, nil))
        elseif frozen_blocks < nblocks then
          check(C.frcnn_roi_pool_backward(delta_outputs[nheads + 1].ptr, fs[1], fs[2], fs[3], post_roi_delta.ptr, pidx, E,
                                          kh, kw, nil))                                 -- :182-185
        end
        end
      else
        for l = 1, nheads do check(C.frcnn_pnet_set_sparse_deltas(native, l, nil, 0)) end
      end

      if rs then
        -- ---- the classification net on sampled proposals: S = F + Bq rows, the first F regress; their rects are constants
        if rs_state.aw == nil then
          local anchors = Anchors.new(pnet, cfg.scales)
          rs_state.aw, rs_state.ah = hip.to_device(anchors.w), hip.to_device(anchors.h)
        end
        local isz = img:size()
        local rec = hip.sample_proposals(rs_state, rs, scratch, outputs, nheads, isz[3], isz[2], d_gt, d_gc, G, bgclass)
        local layers, nl
        if not align then
          nl = #localizer.layers
          layers = ffi.new('int[?]', 6 * nl)
          for i, l in ipairs(localizer.layers) do
            local o = 6 * (i - 1)
            layers[o], layers[o + 1], layers[o + 2], layers[o + 3], layers[o + 4], layers[o + 5] = l.kW, l.kH, l.dW, l.dH, l.padW, l.padH
          end
        end
        if rs.source == 'hard' then
          -- online hard example mining: the N labelled candidates are pooled (no arg-max record) and scored in evaluate mode --
          -- nothing is drawn, no state of the net changes -- and the rows of largest loss become the training tables
          local N = rec.counts[3] + rec.counts[4]
          local score
          if N > 0 then
            local hin = hip.view(scratch('rh_cinput', 4 * N * D).ptr, { N, D })
            if align then
              check(C.frcnn_roi_align_forward(fm.ptr, fs[1], fs[2], fs[3], rec.roi, nil, N, inv_sx, inv_sy, kh, kw, sampling,
                                              hin.ptr, nil))
            else
              local hwins = ffi.cast('int*', scratch('rh_wins', 16 * N).ptr)
              check(C.frcnn_roi_windows(rec.roi, nil, N, layers, nl, fs[2], fs[3], hwins, nil))
              check(C.frcnn_roi_pool_forward(fm.ptr, fs[1], fs[2], fs[3], hwins, N, kh, kw, hin.ptr, nil, nil))
            end
            score = cnet:score(hin, hip.view(scratch('rh_crout', 16 * N).ptr, { N, 4 }),
                               hip.view(scratch('rh_ccout', 4 * N * ncls).ptr, { N, ncls }),
                               model.box_per_class and { 'float', rec.cctarget } or nil)   -- (the loss a row would be trained on)
          end
          rec = hip.mine_hard(rs, rec, scratch, N, score and score[1].ptr, score and score[2].ptr, ncls, cl_desc)
          stats.hard = stats.hard or {}
          table.insert(stats.hard, rec.hard)
        end
        stats.rois = stats.rois or {}
        table.insert(stats.rois, rec.counts)
        F_rows = rec.counts[3]
        local S = rec.counts[3] + rec.counts[4]
        if S == 0 then
          cnet.seed = (cnet.seed or 0) + 1
          check(C.frcnn_pnet_anchor_loss_wait(native, nil))
        else
          local cinput = hip.view(scratch('cinput', 4 * S * D).ptr, { S, D })
          local pidx
          if align then
            check(C.frcnn_roi_align_forward(fm.ptr, fs[1], fs[2], fs[3], rec.roi, nil, S, inv_sx, inv_sy, kh, kw, sampling,
                                            cinput.ptr, nil))
          else
            local dwins = ffi.cast('int*', scratch('rs_wins', 16 * S).ptr)
            pidx = ffi.cast('int*', scratch('pidx', 4 * S * D).ptr)
            check(C.frcnn_roi_windows(rec.roi, nil, S, layers, nl, fs[2], fs[3], dwins, nil))
            check(C.frcnn_roi_pool_forward(fm.ptr, fs[1], fs[2], fs[3], dwins, S, kh, kw, cinput.ptr, pidx, nil))
          end
          local coutputs = cnet:forward(cinput, model.box_per_class and { 'float', rec.cctarget } or nil)
          local crout, ccout = coutputs[1], coutputs[2]
          local crdelta = hip.view(scratch('crdelta', 16 * S).ptr, { S, 4 })
          local ccdelta = hip.view(scratch('ccdelta', 4 * S * ncls).ptr, { S, ncls })
          check(C.frcnn_pnet_anchor_loss_wait(native, nil))
          if cl_desc == nil then
            check(C.frcnn_cnet_losses(crout.ptr, rec.crtarget, ccout.ptr, rec.cctarget, S, F_rows, ncls, crdelta.ptr, ccdelta.ptr,
                                      ffi.cast('double*', acc.ptr) + 4, nil))
          else
            hip.cnet_losses(cl_desc, scratch, crout.ptr, rec.crtarget, ccout.ptr, rec.cctarget, S, F_rows, ncls, crdelta.ptr,
                            ccdelta.ptr, ffi.cast('double*', acc.ptr) + 4)
          end
          local post_roi_delta = cnet:backward(cinput, { crdelta, ccdelta })
          if frozen_blocks < nblocks and align then
            check(C.frcnn_roi_align_backward(delta_outputs[nheads + 1].ptr, fs[1], fs[2], fs[3], post_roi_delta.ptr, rec.roi, nil, S,
                                             inv_sx, inv_sy, kh, kw, sampling, nil))
          elseif frozen_blocks < nblocks then
            check(C.frcnn_roi_pool_backward(delta_outputs[nheads + 1].ptr, fs[1], fs[2], fs[3], post_roi_delta.ptr, pidx, S, kh, kw,
                                            nil))
          end
        end
      end

      pnet:backward(img, delta_outputs)                                 -- :189
      reg_count = reg_count + npos                                      -- :194-198
      cls_count = cls_count + npos + nneg
      creg_count = creg_count + F_rows                                  -- (sampled proposals: the foreground rows regress)
      ccls_count = ccls_count + 1
    end

    -- ---- data parallel (SURVEY 8e): sum the flat gradient, the loss accumulators and the counts over the ranks,
    -- between the last pnet:backward and gradient:div (:197-200) ------------------------------------------------
    if hip.comm then
      local counts = ffi.new('double[4]', cls_count, reg_count, creg_count, ccls_count)
      check(C.frcnn_memcpy_h2d(acc.ptr + 16, counts, 16, nil))          -- slots 2, 3 ...
      check(C.frcnn_memcpy_h2d(acc.ptr + 48, counts + 2, 16, nil))      -- ... and 6, 7 of the 8 accumulators
      if ranges then                                    -- staged training: the trainable slices only
        for _, r in ipairs(ranges) do
          check(C.frcnn_allreduce_f32(hip.comm, ffi.cast('float*', gradient.ptr) + r[1], r[2] - r[1], nil))
        end
      else
        check(C.frcnn_allreduce_f32(hip.comm, gradient.ptr, gradient.n, nil))
      end
      check(C.frcnn_allreduce_f64(hip.comm, ffi.cast('double*', acc.ptr), 8, nil))
    end
    check(C.frcnn_memcpy_d2h(acc_host, acc.ptr, 64, nil))
    check(C.frcnn_stream_sync(nil))
    if hip.comm then
      cls_count, reg_count, creg_count, ccls_count = acc_host[2], acc_host[3], acc_host[6], acc_host[7]
    end
    local cls_loss, reg_loss, creg_loss, ccls_loss = acc_host[0], acc_host[1], acc_host[4], acc_host[5]

    gradient:div(cls_count)                                             -- :200

    local pcls = cls_loss / cls_count                                   -- :202-205
    local preg = reg_loss / reg_count
    local dcls = ccls_loss / ccls_count
    local dreg = creg_loss / creg_count
    if not classification then dcls, dreg = 0 / 0, 0 / 0 end           -- (no detector stage was computed)
    print(string.format('prop: cls: %f (%d), reg: %f (%d); det: cls: %f, reg: %f',
      pcls, cls_count, preg, reg_count, dcls, dreg))                    -- :207-209
    table.insert(stats.pcls, pcls)                                      -- :211-214
    table.insert(stats.preg, preg)
    table.insert(stats.dcls, dcls)
    table.insert(stats.dreg, dreg)

    local loss = pcls + preg                                            -- :216-217
    return loss, gradient
  end

  return lossAndGradient
end
