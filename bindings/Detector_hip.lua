-- Detector_hip.lua -- drop-in for the reference's Detector.lua on libfrcnn_hip.so: the same class (`Detector(model)`,
-- `:detect(input) -> winners`, each winner a table { p, a, r, l, r2, class, confidence }), the same pipeline and
-- thresholds (p > 0.95, NMS 0.25, class ~= background and p > 0.2, per-class NMS 0.1) -- but the 26 544-iteration
-- Lua loop of Detector.lua:39-66 is one scan + compaction kernel (frcnn_rpn_scan), the per-candidate pooling loop
-- (:94-98) one batched kernel, and the first NMS runs on the device.  Both NMS calls of the reference pass a tensor as
-- `scores`, which nms.lua:37-43 ignores: boxes are processed by descending max-y.  That behaviour is reproduced.
-- 1:1 with the tested Python host mirror (faster-rcnn.torch_amd/Detector.py); checked statically, not executed here.
--
--   main.lua:  require 'Detector'  ->  require 'Detector_hip'
local ffi = require 'ffi'
local hip = require 'frcnn_hip'
require 'Anchors'            -- the reference's own files, unchanged
require 'Localizer'
require 'objective_hip'      -- extract_roi_pooling_input
local C, check = hip.C, hip.check

local ASPECTS = 3   -- anchors per map position (Anchors.lua:108-109)

local Detector = torch.class('Detector')

function Detector:__init(model)                                         -- Detector.lua:8-15
  local cfg = model.cfg
  self.model = model
  self.anchors = Anchors.new(model.pnet, cfg.scales)
  self.nheads = #model.anchor_nets
  self.localizer = Localizer.new(model.pnet.outnode.children[self.nheads + 1])
  -- the fp32 tables of Anchors.lua:18-19, resident on the device for the scan
  self.aw = hip.to_device(self.anchors.w)
  self.ah = hip.to_device(self.anchors.h)
  self.scratch = hip.scratch()
end

function Detector:detect(input)                                         -- Detector.lua:17-141
  local model = self.model
  local cfg = model.cfg
  local pnet = model.pnet
  local cnet = model.cnet
  local kh, kw = cfg.roi_pooling.kh, cfg.roi_pooling.kw
  local bgclass = cfg.class_count + 1
  local ncls = cfg.class_count + 1
  local cnet_input_planes = model.layers[#model.layers].filters
  local D = kh * kw * cnet_input_planes
  local scratch = self.scratch

  local input_size = input:size()
  pnet:evaluate()                                                       -- :31
  input = hip.to_device(input)                                          -- :32
  local outputs = pnet:forward(input)                                   -- :33

  -- ---- :39-66 on the device: log-softmax of every anchor's two logits, p > 0.95, decode, overlap test, compaction
  local Hs, Ws, maps = ffi.new('int[4]'), ffi.new('int[4]'), ffi.new('const float*[4]')
  for i = 1, 4 do
    local s = outputs[i]:size()
    Hs[i - 1], Ws[i - 1], maps[i - 1] = s[2], s[3], outputs[i].ptr
  end
  local cap = 0   -- every anchor of the four maps may pass: the buffers hold them all (vgg_large 1000x600: 45 015)
  for i = 0, 3 do cap = cap + ASPECTS * Hs[i] * Ws[i] end
  local wsb = tonumber(C.frcnn_rpn_scan_workspace_bytes(Hs, Ws))
  local ws = scratch('scan_ws', wsb)
  local mp = ffi.cast('float*', scratch('match_p', 4 * cap).ptr)
  local mi = ffi.cast('int*', scratch('match_idx', 16 * cap).ptr)
  local mr = ffi.cast('double*', scratch('match_rect', 32 * cap).ptr)
  local mb = ffi.cast('float*', scratch('match_box', 16 * cap).ptr)
  -- counts (device int[4]): matches, NMS candidates, candidates that pass the class test, winners
  local cnt = ffi.cast('int*', scratch('counts', 16).ptr)
  check(C.frcnn_rpn_scan(maps, Hs, Ws, self.aw.ptr, self.ah.ptr, input_size[3], input_size[2], 0.95, cap, mp, mi, mr, mb,
                         cnt, ws.ptr, wsb, nil))
  -- NON-MAXIMUM SUPPRESSION (:74-85) on the device, the match count read from DEVICE memory (no round trip between scan
  -- and NMS); the score tensor is ignored by nms.lua -> key = max-y
  -- (launch and workspace sized for a bound on the matches, not for every anchor of the maps; a frame with more matches
  -- repeats the pass sized by the count just read)
  local ncap = math.min(cap, 16384)
  local nwsb = tonumber(C.frcnn_nms_workspace_bytes(ncap))
  local nws = scratch('nms_ws', nwsb)
  local dpick = ffi.cast('long long*', scratch('pick', 8 * cap).ptr)
  check(C.frcnn_nms_device_n(mb, ncap, cnt, 4, 0.25, 0, 0, nil, dpick, cnt + 1, nws.ptr, nwsb, nil))
  local count = ffi.new('int[2]')
  check(C.frcnn_memcpy_d2h(count, cnt, 8, nil))                          -- ---- read-back 1 of 2: two counts
  check(C.frcnn_stream_sync(nil))
  if count[0] > cap then
    error(string.format('Detector: %d anchors pass p > 0.95, more than the %d the maps hold', count[0], cap))
  end
  if count[0] > ncap then
    nwsb = tonumber(C.frcnn_nms_workspace_bytes(count[0]))
    nws = scratch('nms_ws_full', nwsb)
    check(C.frcnn_nms_device(mb, count[0], 4, 0.25, 0, 0, dpick, cnt + 1, nws.ptr, nwsb, nil))
    check(C.frcnn_memcpy_d2h(count + 1, cnt + 1, 4, nil))
    check(C.frcnn_stream_sync(nil))
  end
  local nm, R = count[0], count[1]

  local winners = {}
  if nm > 0 then                                                        -- :71
    print(string.format('candidates: %d', R))                           -- :87
    -- REGION CLASSIFICATION (:90-101): every candidate's window (objective.lua:5-13 for all of them in one kernel), one
    -- pooling launch (no indices: there is no backward pass), one cnet pass
    cnet:evaluate()
    local fm = outputs[self.nheads + 1]
    local fs = fm:size()
    local nl = #self.localizer.layers
    local layers = ffi.new('int[?]', 6 * nl)
    for i, l in ipairs(self.localizer.layers) do
      local o = 6 * (i - 1)
      layers[o], layers[o + 1], layers[o + 2], layers[o + 3], layers[o + 4], layers[o + 5] = l.kW, l.kH, l.dW, l.dH, l.padW, l.padH
    end
    local dwins = ffi.cast('int*', scratch('wins', 16 * R).ptr)
    check(C.frcnn_roi_windows(mr, dpick, R, layers, nl, fs[2], fs[3], dwins, nil))
    local cinput = hip.view(scratch('cinput', 4 * R * D).ptr, { R, D })
    check(C.frcnn_roi_pool_forward(fm.ptr, fs[1], fs[2], fs[3], dwins, R, kh, kw, cinput.ptr, nil, nil))
    local coutputs = cnet:forward(cinput)                               -- :101
    local bbox_out, cls_out = coutputs[1], coutputs[2]
    local dcls = ffi.cast('int*', scratch('cls', 4 * R).ptr)
    local dconf = ffi.cast('float*', scratch('conf', 4 * R).ptr)
    check(C.frcnn_cnet_decode(cls_out.ptr, R, ncls, dcls, dconf, nil))  -- :110-113 (arg-max of the log-probs)
    -- :106-122 on the device: class test, r2 = Anchors.anchorToInput(r, bbox) in double, survivors compacted in order
    local dbb = ffi.cast('float*', scratch('bb5', 20 * R).ptr)
    local dkc = ffi.cast('int*', scratch('bbcls', 4 * R).ptr)
    local dkeep = ffi.cast('int*', scratch('keep_row', 4 * R).ptr)
    local dr2 = ffi.cast('double*', scratch('r2', 32 * R).ptr)
    check(C.frcnn_detect_post(dcls, dconf, bbox_out.ptr, mr, dpick, R, bgclass, 0.2, dbb, dkc, dkeep, dr2, cnt + 2, nil))
    -- per-class NMS (:125-136), every class in ONE device pass: rows only suppress rows of their own class; a stable
    -- partition of the picks by class is, per class, exactly nms(bb, 0.1, bb[{{}, 5}]) -- the score tensor is ignored by
    -- nms.lua:42, the key is max-y.  The survivor count is read from device memory.
    local cwsb = tonumber(C.frcnn_nms_workspace_bytes(R))
    local cws = scratch('nms_ws2', cwsb)
    local cpick = ffi.cast('long long*', scratch('wpick', 8 * R).ptr)
    check(C.frcnn_nms_device_n(dbb, R, cnt + 2, 5, 0.1, 0, 0, dkc, cpick, cnt + 3, cws.ptr, cwsb, nil))
    -- one record of 16 doubles per winner behind a 128-byte header that carries the four counts
    local out = ffi.cast('double*', scratch('winners', 128 * (R + 1)).ptr)
    check(C.frcnn_memcpy_d2d(out, cnt, 16, nil))
    check(C.frcnn_detect_gather(cpick, cnt + 3, R, dkeep, dkc, dbb, dr2, dpick, mp, mr, mi, out + 16, nil))
    local h = ffi.new('double[?]', 16 * (R + 1))
    check(C.frcnn_memcpy_d2h(h, out, 128 * (R + 1), nil))                -- ---- read-back 2 of 2: the winner table
    check(C.frcnn_stream_sync(nil))
    local nwin = ffi.cast('int*', h)[3]
    -- classes in ascending order (the reference iterates with pairs(): unspecified), pick order within a class
    local byclass, classes = {}, {}
    for q = 1, nwin do
      local v = h + 16 * q
      local l, a, y, x = tonumber(v[12]), tonumber(v[13]), tonumber(v[14]), tonumber(v[15])
      local det = { p = v[3], a = self.anchors:get(l, a, y, x), l = l, r = Rect.new(v[4], v[5], v[6], v[7]),
                    r2 = Rect.new(v[8], v[9], v[10], v[11]), class = tonumber(v[0]), confidence = v[2] }
      if not byclass[det.class] then
        byclass[det.class] = {}
        classes[#classes + 1] = det.class
      end
      table.insert(byclass[det.class], det)
    end
    table.sort(classes)
    for _, ci in ipairs(classes) do
      for _, x in ipairs(byclass[ci]) do table.insert(winners, x) end
    end
  end

  return winners
end

-- Detector:detect_batch(inputs, shared_cnet) -- detect() for a list of frames of ONE size: a list with one entry per frame,
-- in order, each what detect(frame) returns.  Chunks of Detector.BATCH frames: the proposal net runs frame by frame (its
-- head maps and last feature map are copied to the frame's slot), then ONE scan, ONE segmented NMS, per frame with
-- candidates the pooling / classification net / class test of detect(), ONE segmented per-class NMS and ONE gather; the
-- host waits twice per chunk instead of twice per frame.  Bit-identical to detect() frame by frame.
-- shared_cnet = true: ONE classification-net pass over the candidates of all frames of a chunk (frame b's rows at the prefix
-- sum of the candidate counts); everything up to the pooled rows stays bit-identical, the net's outputs agree with detect()'s
-- within the net's own error only (input scale and Linear form depend on the whole tensor / the row count).
-- 1:1 with Detector.detect_batch of the Python host mirror.
Detector.BATCH = 8

function Detector:detect_batch(inputs, shared_cnet)
  local nframes = #inputs
  for i = 2, nframes do                                                 -- refused before anything is queued
    local a, b = inputs[1]:size(), inputs[i]:size()
    if a[1] ~= b[1] or a[2] ~= b[2] or a[3] ~= b[3] then
      error('Detector:detect_batch: frames of different sizes in one call')
    end
  end
  local results = {}
  local lo = 1
  while lo <= nframes do
    local chunk = {}
    for i = lo, math.min(lo + Detector.BATCH - 1, nframes) do chunk[#chunk + 1] = inputs[i] end
    for _, winners in ipairs(self:detect_chunk(chunk, shared_cnet)) do results[#results + 1] = winners end
    lo = lo + Detector.BATCH
  end
  return results
end

function Detector:detect_chunk(frames, shared)
  local model = self.model
  local cfg = model.cfg
  local pnet = model.pnet
  local cnet = model.cnet
  local kh, kw = cfg.roi_pooling.kh, cfg.roi_pooling.kw
  local bgclass = cfg.class_count + 1
  local ncls = cfg.class_count + 1
  local D = kh * kw * model.layers[#model.layers].filters
  local scratch = self.scratch
  local B = #frames

  -- counts (device int[4][B]): per frame matches, NMS candidates, candidates that pass the class test, winners
  local cnt = ffi.cast('int*', scratch('b_counts', 16 * B).ptr)
  local input_size = frames[1]:size()
  pnet:evaluate()
  -- ---- 1. per frame: the proposal net; its outputs are copied to the frame's slot (the net reuses its output buffers)
  local Hs, Ws, maps, hoff = ffi.new('int[4]'), ffi.new('int[4]'), ffi.new('const float*[4]'), { 0 }
  local slot, fslot, heads, fms, fs
  for b = 0, B - 1 do
    local outputs = pnet:forward(hip.to_device(frames[b + 1]))
    if b == 0 then
      for i = 1, 4 do
        local s = outputs[i]:size()
        Hs[i - 1], Ws[i - 1] = s[2], s[3]
        hoff[i + 1] = hoff[i] + math.floor((s[1] * s[2] * s[3] + 63) / 64) * 64
      end
      slot = hoff[5]
      fs = outputs[self.nheads + 1]:size()
      fslot = math.floor((fs[1] * fs[2] * fs[3] + 63) / 64) * 64
      heads = ffi.cast('float*', scratch('b_heads', 4 * B * slot).ptr)
      fms = ffi.cast('float*', scratch('b_fm', 4 * B * fslot).ptr)
      for i = 0, 3 do maps[i] = heads + hoff[i + 1] end
    end
    for i = 1, 4 do
      check(C.frcnn_memcpy_d2d(heads + b * slot + hoff[i], outputs[i].ptr, 4 * 18 * Hs[i - 1] * Ws[i - 1], nil))
    end
    check(C.frcnn_memcpy_d2d(fms + b * fslot, outputs[self.nheads + 1].ptr, 4 * fs[1] * fs[2] * fs[3], nil))
  end
  -- ---- 2. ONE scan over the B slots: frame b's matches at rows [b * cap, b * cap + n_b)
  local cap = 0
  for i = 0, 3 do cap = cap + ASPECTS * Hs[i] * Ws[i] end
  local wsb = tonumber(C.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, B))
  local ws = scratch('b_scan_ws', wsb)
  local mp = ffi.cast('float*', scratch('b_match_p', 4 * B * cap).ptr)
  local mi = ffi.cast('int*', scratch('b_match_idx', 16 * B * cap).ptr)
  local mr = ffi.cast('double*', scratch('b_match_rect', 32 * B * cap).ptr)
  local mb = ffi.cast('float*', scratch('b_match_box', 16 * B * cap).ptr)
  check(C.frcnn_rpn_scan_batch(maps, Hs, Ws, B, slot, self.aw.ptr, self.ah.ptr, input_size[3], input_size[2], 0.95, cap,
                               mp, mi, mr, mb, cnt, ws.ptr, wsb, nil))
  -- ---- 3. ONE segmented NMS, the match counts read from device memory, sized for the bound of detect()
  local ncap = math.min(cap, 16384)
  local nwsb = tonumber(C.frcnn_nms_batch_workspace_bytes(B, ncap))
  local nws = scratch('b_nms_ws', nwsb)
  local dpick = ffi.cast('long long*', scratch('b_pick', 8 * B * cap).ptr)
  check(C.frcnn_nms_device_batch(mb, B, cap, ncap, cnt, 4, 0.25, 0, 0, nil, dpick, cnt + B, nws.ptr, nwsb, nil))
  local count = ffi.new('int[?]', 2 * B)
  check(C.frcnn_memcpy_d2h(count, cnt, 8 * B, nil))                      -- ---- read-back 1 of 2: B pairs of counts
  check(C.frcnn_stream_sync(nil))
  local Rmax = 0
  for b = 0, B - 1 do
    if count[b] > cap then
      error(string.format('Detector: %d anchors pass p > 0.95, more than the %d the maps hold', count[b], cap))
    end
    if count[b] > ncap then                                             -- the frame repeats its NMS alone, as in detect()
      local fwsb = tonumber(C.frcnn_nms_workspace_bytes(count[b]))
      local fws = scratch('nms_ws_full', fwsb)
      check(C.frcnn_nms_device(mb + 4 * b * cap, count[b], 4, 0.25, 0, 0, dpick + b * cap, cnt + B + b, fws.ptr, fwsb, nil))
      check(C.frcnn_memcpy_d2h(count + B + b, cnt + B + b, 4, nil))
      check(C.frcnn_stream_sync(nil))
    end
    if count[b] > 0 then Rmax = math.max(Rmax, count[B + b]) end
  end
  local results = {}
  for b = 1, B do results[b] = {} end
  if Rmax == 0 then return results end                                  -- :71, every frame
  -- ---- 4. per frame with candidates: REGION CLASSIFICATION (:90-101) and the class test (:106-122) into its segment
  cnet:evaluate()
  local nl = #self.localizer.layers
  local layers = ffi.new('int[?]', 6 * nl)
  for i, l in ipairs(self.localizer.layers) do
    local o = 6 * (i - 1)
    layers[o], layers[o + 1], layers[o + 2], layers[o + 3], layers[o + 4], layers[o + 5] = l.kW, l.kH, l.dW, l.dH, l.padW, l.padH
  end
  local dwins = ffi.cast('int*', scratch('wins', 16 * Rmax).ptr)
  local dcls = ffi.cast('int*', scratch('cls', 4 * Rmax).ptr)
  local dconf = ffi.cast('float*', scratch('conf', 4 * Rmax).ptr)
  local dbb = ffi.cast('float*', scratch('b_bb5', 20 * B * Rmax).ptr)
  local dkc = ffi.cast('int*', scratch('b_bbcls', 4 * B * Rmax).ptr)
  local dkeep = ffi.cast('int*', scratch('b_keep_row', 4 * B * Rmax).ptr)
  local dr2 = ffi.cast('double*', scratch('b_r2', 32 * B * Rmax).ptr)
  -- first row of frame b in the shared pass's input / output: the prefix sum of the candidate counts
  local row0, total = {}, 0
  for b = 0, B - 1 do
    if count[b] > 0 then
      row0[b] = total
      total = total + count[B + b]
    end
  end
  local cbuf = ffi.cast('float*', shared and scratch('b_cinput', 4 * total * D).ptr or scratch('cinput', 4 * Rmax * D).ptr)
  local function pooled(b)              -- ROI windows and ROI pooling of frame b -> its input rows
    local R = count[B + b]
    check(C.frcnn_roi_windows(mr + 4 * b * cap, dpick + b * cap, R, layers, nl, fs[2], fs[3], dwins, nil))
    local cinput = hip.view(shared and (cbuf + row0[b] * D) or cbuf, { R, D })
    check(C.frcnn_roi_pool_forward(fms + b * fslot, fs[1], fs[2], fs[3], dwins, R, kh, kw, cinput.ptr, nil, nil))
    return cinput
  end
  local all_bbox, all_cls
  if shared then
    for b = 0, B - 1 do
      if count[b] > 0 then pooled(b) end
    end
    local coutputs = cnet:forward(hip.view(cbuf, { total, D }))         -- :101, all frames
    all_bbox, all_cls = ffi.cast('float*', coutputs[1].ptr), ffi.cast('float*', coutputs[2].ptr)
  end
  for b = 0, B - 1 do
    local R = count[B + b]
    if count[b] > 0 then
      print(string.format('candidates: %d', R))                         -- :87
      local bbox_ptr, cls_ptr
      if shared then
        bbox_ptr, cls_ptr = all_bbox + 4 * row0[b], all_cls + ncls * row0[b]
      else
        local coutputs = cnet:forward(pooled(b))                        -- :101
        bbox_ptr, cls_ptr = coutputs[1].ptr, coutputs[2].ptr
      end
      check(C.frcnn_cnet_decode(cls_ptr, R, ncls, dcls, dconf, nil))
      check(C.frcnn_detect_post(dcls, dconf, bbox_ptr, mr + 4 * b * cap, dpick + b * cap, R, bgclass, 0.2,
                                dbb + 5 * b * Rmax, dkc + b * Rmax, dkeep + b * Rmax, dr2 + 4 * b * Rmax, cnt + 2 * B + b, nil))
    else
      check(C.frcnn_zero(cnt + 2 * B + b, 4, nil))                      -- no candidates: an empty segment of the per-class NMS
    end
  end
  -- ---- 5. ONE segmented per-class NMS (one segment per frame), ONE gather of every frame's winner records behind a
  --         header of the frame's four counts
  local cwsb = tonumber(C.frcnn_nms_batch_workspace_bytes(B, Rmax))
  local cws = scratch('b_nms_ws2', cwsb)
  local cpick = ffi.cast('long long*', scratch('b_wpick', 8 * B * Rmax).ptr)
  check(C.frcnn_nms_device_batch(dbb, B, Rmax, Rmax, cnt + 2 * B, 5, 0.1, 0, 0, dkc, cpick, cnt + 3 * B, cws.ptr, cwsb, nil))
  local out = ffi.cast('double*', scratch('b_winners', 128 * B * (Rmax + 1)).ptr)
  check(C.frcnn_detect_gather_batch(cpick, cnt, B, Rmax, dkeep, dkc, dbb, dr2, dpick, cap, mp, mr, mi, out, nil))
  local h = ffi.new('double[?]', 16 * B * (Rmax + 1))
  check(C.frcnn_memcpy_d2h(h, out, 128 * B * (Rmax + 1), nil))           -- ---- read-back 2 of 2: every frame's winner table
  check(C.frcnn_stream_sync(nil))
  for b = 0, B - 1 do
    local tab = h + 16 * b * (Rmax + 1)
    local nwin = ffi.cast('int*', tab)[3]
    -- classes in ascending order (the reference iterates with pairs(): unspecified), pick order within a class
    local byclass, classes = {}, {}
    for q = 1, nwin do
      local v = tab + 16 * q
      local l, a, y, x = tonumber(v[12]), tonumber(v[13]), tonumber(v[14]), tonumber(v[15])
      local det = { p = v[3], a = self.anchors:get(l, a, y, x), l = l, r = Rect.new(v[4], v[5], v[6], v[7]),
                    r2 = Rect.new(v[8], v[9], v[10], v[11]), class = tonumber(v[0]), confidence = v[2] }
      if not byclass[det.class] then
        byclass[det.class] = {}
        classes[#classes + 1] = det.class
      end
      table.insert(byclass[det.class], det)
    end
    table.sort(classes)
    for _, ci in ipairs(classes) do
      for _, x in ipairs(byclass[ci]) do table.insert(results[b + 1], x) end
    end
  end
  return results
end
