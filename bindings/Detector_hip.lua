-- Detector_hip.lua -- drop-in for the reference's Detector.lua on libfrcnn_hip.so: the same class (`Detector(model)`,
-- `:detect(input) -> winners`, each winner a table { p, a, r, l, r2, class, confidence }), the same pipeline and
-- thresholds (p > 0.95, NMS 0.25, class ~= background and p > 0.2, per-class NMS 0.1) -- but the 26 544-iteration
-- Lua loop of Detector.lua:39-66 is one scan + compaction kernel (frcnn_rpn_scan_batch), the per-candidate pooling loop
-- (:94-98) one batched kernel, and the first NMS runs on the device.  Both NMS calls of the reference pass a tensor as
-- `scores`, which nms.lua:37-43 ignores: boxes are processed by descending max-y.  That behaviour is reproduced.
-- There is ONE pipeline, written for a chunk of B frames (first_stage + detect_chunk: ONE scan, frcnn_nms_device_batch twice,
-- frcnn_detect_gather_batch; frcnn_nms_device for a frame over the first NMS's bound), with ONE front: every frame's slot
-- offsets, feature-map size and anchor count come from its size's layout (Detector:layout, host arithmetic, cached per size),
-- the chunk's strides are those of its largest frame, and the sizes pick the scan -- frcnn_rpn_scan_batch for a chunk of one
-- size, frcnn_rpn_scan_ragged for one that mixes sizes under detect_batch's opts.mixed_sizes:
-- detect_batch runs it on chunks of Detector.BATCH frames, detect(input) on the chunk { input }, which reads the proposal
-- net's outputs where the net left them (no device copies); proposals(input) runs its first stage.
-- 1:1 with the tested Python host mirror (faster-rcnn.torch_amd/Detector.py); checked statically, not executed here.
--
-- Not in the reference, off by default: cfg.proposals = { order = 'y2' | 'score', pre_nms_top_n = K, post_nms_top_n = M }
-- (main.lua calls Detector(model) unchanged, so the settings ride on the model's cfg; Detector.proposal_settings).
-- Likewise cfg.nms = { method = 'hard' | 'linear' | 'gaussian', overlap, sigma, min_score } (Detector.nms_settings): Soft-NMS in
-- the per-class pass.  Under 'linear' or 'gaussian' a winner's confidence is its DECAYED log-score, the one it was ranked by.
-- And cfg.box_voting = { overlap = 0.5, weight = 'score' | 'uniform' } (Detector.box_voting_settings): behind the per-class pass a
-- winner's r2 becomes the weighted mean of the r2 of its class's survivors that overlap it; nothing else about a winner changes.
-- And cfg.scoring = { classes = 'top' | 'all', min_confidence = 0.2, max_detections = M, boxes = 'candidate' | 'class' }
-- (Detector.scoring_settings, Detector.scoring_boxes; boxes = 'class': the box of its own class for every class row): the class
-- test as ONE frcnn_detect_classes_batch launch per chunk; 'all' scores a candidate under every foreground class over the threshold.
-- And cfg.tta = { hflip = false, scales = { 1.0 } } (Detector.tta_settings): test-time augmentation.  A frame is detected on V
-- views of itself -- per scale the rescaled frame and, under hflip, its mirror --, which are the SEGMENTS of the chunk; behind the
-- class test ONE frcnn_detect_merge_views launch makes one segment per frame of them, in the frame's coordinates, and the per-class
-- pass, voting and the gather run on those.  A winner gains `view` (0-based); its r2 is in the frame's coordinates, its p, r and a
-- describe the anchor in the view's, its candidate row counts through the views' candidates in view order.
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
  self.proposal_order, self.pre_nms_top_n, self.post_nms_top_n = Detector.proposal_settings(self.model.cfg.proposals)
  self.nms_method, self.nms_overlap, self.nms_sigma, self.nms_min_score = Detector.nms_settings(self.model.cfg.nms)
  self.vote_overlap, self.vote_weight = Detector.box_voting_settings(self.model.cfg.box_voting)
  self:set_scoring(self.model.cfg.scoring)
  self:set_tta(self.model.cfg.tta)
end

-- cfg.tta -> nil (the key is absent: one forward pass over the frame) or hflip, scales (validated on the host, before any device
-- call).  The frame is detected on V = #scales * (hflip and 2 or 1) views of itself and the per-class pass -- hard or soft NMS,
-- voting -- runs over the union of what they found.
--   hflip   false (default) or true: behind every scale's view comes its left-right mirror
--   scales  a non-empty list of distinct positive numbers, default { 1.0 }: per scale s, in the order given, an H x W frame is
--           rescaled to max(1, floor(H * s)) x max(1, floor(W * s)) (BatchIterator.lua:52); s = 1 is the frame itself
-- A table whose only view is the frame itself ({}, { scales = { 1 } }) is off: the launches and results of the key absent.
function Detector.tta_settings(t)
  if t == nil then return nil end
  if type(t) ~= 'table' then error('cfg.tta must be a table of {hflip, scales}') end
  for k, _ in pairs(t) do
    if k ~= 'hflip' and k ~= 'scales' then error('cfg.tta: unknown key ' .. tostring(k)) end
  end
  local hflip = t.hflip
  if hflip == nil then hflip = false end
  if type(hflip) ~= 'boolean' then error('cfg.tta.hflip must be true or false') end
  local scales = t.scales
  if scales == nil then scales = { 1.0 } end
  if type(scales) ~= 'table' or #scales == 0 then error('cfg.tta.scales must be a non-empty list of numbers') end
  local n = 0
  for _, _ in pairs(scales) do n = n + 1 end
  if n ~= #scales then error('cfg.tta.scales must be a non-empty list of numbers') end
  local out = {}
  for i, v in ipairs(scales) do
    if type(v) ~= 'number' then error('cfg.tta.scales: not a number') end
    if not (v > 0 and v < math.huge) then error('cfg.tta.scales must be finite and > 0') end
    for j = 1, i - 1 do
      if out[j] == v then error('cfg.tta.scales: ' .. v .. ' is given twice') end
    end
    out[i] = v
  end
  return hflip, out
end

-- Makes a table as tta_settings takes it this Detector's setting from the next frame on (nil: no augmentation)
function Detector:set_tta(t)
  self.tta_hflip, self.tta_scales = Detector.tta_settings(t)
end

-- The views of the frames of `sizes` ({ 3, H, W } each) -> nil when the setting is off -- absent, or the frame alone --, else per
-- frame a list of { scale, flip, dH, dW }, scale-major, the unmirrored view first.  Refused on the host, before anything is queued:
-- more views a frame than Detector.BATCH segments, and a view too small for the proposal net (a head map without positions)
function Detector:view_lists(sizes)
  local scales = self.tta_scales
  if scales == nil or (not self.tta_hflip and #scales == 1 and scales[1] == 1) then return nil end
  local V = #scales * (self.tta_hflip and 2 or 1)
  if V > Detector.BATCH then
    error(string.format('cfg.tta: %d views a frame, more than the %d segments of a chunk (Detector.BATCH)', V, Detector.BATCH))
  end
  local lists = {}
  for f, size in ipairs(sizes) do
    local H, W = size[2], size[3]
    local list = {}
    for _, sc in ipairs(scales) do
      local dH, dW = H, W
      if sc ~= 1 then dH, dW = math.max(1, math.floor(H * sc)), math.max(1, math.floor(W * sc)) end
      for i = 1, 4 do
        local hw = self:layout(dH, dW).hw[i]
        if hw[1] < 1 or hw[2] < 1 then
          error(string.format("cfg.tta: scale %g makes a %dx%d view, too small for the proposal net's head maps", sc, dW, dH))
        end
      end
      list[#list + 1] = { sc, false, dH, dW }
      if self.tta_hflip then list[#list + 1] = { sc, true, dH, dW } end
    end
    lists[f] = list
  end
  return lists, V
end

-- The views of frame f (0-based) of a chunk, in scratch buffers of this Detector: per scale the rescaled frame (frcnn_image_scale;
-- scale 1 is the frame itself: no launch, no copy), then -- hflip -- its mirror (frcnn_image_crop_flip over the whole view)
function Detector:make_views(frame, list, f, prefix, out)
  local scratch = self.scratch
  local x = hip.to_device(frame)
  local size = x:size()
  local H, W = size[2], size[3]
  local base
  for i, v in ipairs(list) do
    local sc, flip, dH, dW = v[1], v[2], v[3], v[4]
    if not flip then
      base = x
      if sc ~= 1 then
        base = hip.view(scratch(prefix .. 'tta_view_' .. f .. '_' .. i, 12 * dH * dW).ptr, { 3, dH, dW })
        local tmp = scratch(prefix .. 'tta_tmp', 12 * H * dW)
        check(C.frcnn_image_scale(x.ptr, 3, H, W, base.ptr, dH, dW, ffi.cast('float*', tmp.ptr), 0, nil))
      end
      out[#out + 1] = base
    else                                               -- (the unmirrored view of this scale came just before)
      local m = hip.view(scratch(prefix .. 'tta_view_' .. f .. '_' .. i, 12 * dH * dW).ptr, { 3, dH, dW })
      check(C.frcnn_image_crop_flip(base.ptr, 3, dH, dW, 0, 0, dW, dH, 1, 0, m.ptr, nil))
      out[#out + 1] = m
    end
  end
end

-- cfg.scoring -> nil (the key is absent: the reference's class test, launch for launch) or classes, min_confidence,
-- max_detections (validated on the host, before any device call).  The setting governs the class test between the classification
-- net and the per-class NMS, which under it is ONE frcnn_detect_classes_batch launch per chunk.
--   classes         'top' (default: the reference -- a candidate is scored under the arg-max of its log-probabilities only, and
--                   dropped when that is the background) or 'all': one row per foreground class whose probability clears
--                   min_confidence, whatever the arg-max is
--   min_confidence  in [0, 1), a probability; default 0.2 (the reference's literal)
--   max_detections  nil or M >= 1: a frame keeps the M winners of highest confidence (ties to the earlier pick), applied on the
--                   host behind read-back 2
-- An empty table is 'top' at 0.2: the results of the key absent, from one launch.
function Detector.scoring_settings(t)
  if t == nil then return nil end
  if type(t) ~= 'table' then error('cfg.scoring must be a table of {classes, min_confidence, max_detections}') end
  for k, _ in pairs(t) do
    if k ~= 'classes' and k ~= 'min_confidence' and k ~= 'max_detections' and k ~= 'boxes' then   -- (boxes: scoring_boxes)
      error('cfg.scoring: unknown key ' .. tostring(k))
    end
  end
  local classes = t.classes
  if classes == nil then classes = 'top' end
  if classes ~= 'top' and classes ~= 'all' then error('cfg.scoring.classes must be "top" or "all"') end
  local min_confidence = t.min_confidence
  if min_confidence == nil then min_confidence = 0.2 end
  if type(min_confidence) ~= 'number' then error('cfg.scoring.min_confidence is not a number') end
  if not (min_confidence >= 0 and min_confidence < 1) then error('cfg.scoring.min_confidence must be in [0, 1)') end
  local M = t.max_detections
  if M ~= nil then
    if type(M) ~= 'number' or M ~= math.floor(M) then error('cfg.scoring.max_detections is not an integer') end
    if M < 1 then error('cfg.scoring.max_detections must be at least 1') end
  end
  return classes, min_confidence, M
end

-- cfg.scoring.boxes -> 'candidate' (default, also without the table: a candidate has ONE box, the net's, and under classes =
-- 'all' all its class rows carry it) or 'class': every emitted row (candidate r, class c) carries the box class c's four
-- regressor rows predict for r -- ONE frcnn_detect_class_boxes_batch launch per chunk behind the class test.  Needs a per-class
-- box head (cfg.box_head.per_class); under classes = 'top' the row's class is the arg-max, whose box the net wrote already: the
-- launches of 'candidate'.  1:1 with scoring_boxes of the Python mirror.
function Detector.scoring_boxes(t)
  if t == nil then return 'candidate' end
  if type(t) ~= 'table' then error('cfg.scoring must be a table of {classes, min_confidence, max_detections, boxes}') end
  local boxes = t.boxes
  if boxes == nil then return 'candidate' end
  if boxes ~= 'candidate' and boxes ~= 'class' then error('cfg.scoring.boxes must be "candidate" or "class"') end
  return boxes
end

-- Makes a table as scoring_settings takes it this Detector's class test from the next frame on (nil: the reference's)
function Detector:set_scoring(t)
  local classes, min_confidence, max_detections = Detector.scoring_settings(t)
  local boxes = Detector.scoring_boxes(t)
  if boxes == 'class' and not self.model.box_per_class then
    error('cfg.scoring.boxes = "class" needs cfg.box_head.per_class = true: a shared box head has one box per candidate')
  end
  -- a per-class box head (cfg.box_head) has one box per (candidate, class); classes = 'all' decodes ONE box per candidate
  if classes == 'all' and self.model.box_per_class and boxes ~= 'class' then
    error('cfg.scoring.classes = "all" cannot be combined with cfg.box_head.per_class = true; cfg.scoring.boxes = "class" gives ' ..
          'every class row the box of its own class')
  end
  self.scoring_classes, self.min_confidence, self.max_detections = classes, min_confidence, max_detections
  self.scoring_box = boxes
end

-- m: the rows a candidate can emit, what the per-row buffers of a chunk are sized by (Rmax * m rows a frame).  'top': 1.  'all':
-- min(ncls - 1, floor(1 / min_confidence) + 1) -- at most floor(1 / c) classes exceed c when the probabilities sum to 1, one more
-- slot covers the rounding of an fp32 log-softmax; ncls - 1 at min_confidence = 0
function Detector:scoring_rows(ncls)
  if self.scoring_classes ~= 'all' then return 1 end
  if self.min_confidence <= 0 then return ncls - 1 end
  return math.min(ncls - 1, math.floor(1 / self.min_confidence) + 1)
end

-- cfg.box_voting -> nil (the key is absent: no voting, the reference's r2) or overlap, weight (validated on the host, before any
-- device call).  Voting runs behind the per-class pass and changes a winner's r2 only: it becomes the weighted mean of the r2 of
-- every survivor of the class test that has the winner's class and overlaps it by an IoU >= overlap, the winner included.
--   overlap  in (0, 1]; default 0.5
--   weight   'score' (default: a voter weighs its confidence as a probability -- the undecayed one, also under a soft per-class
--            NMS) or 'uniform' (every voter weighs 1)
-- An empty table turns voting on with the defaults.
function Detector.box_voting_settings(t)
  if t == nil then return nil end
  if type(t) ~= 'table' then error('cfg.box_voting must be a table of {overlap, weight}') end
  for k, _ in pairs(t) do
    if k ~= 'overlap' and k ~= 'weight' then error('cfg.box_voting: unknown key ' .. tostring(k)) end
  end
  local weight = t.weight
  if weight == nil then weight = 'score' end
  if weight ~= 'score' and weight ~= 'uniform' then error('cfg.box_voting.weight must be "score" or "uniform"') end
  local overlap = t.overlap
  if overlap == nil then overlap = 0.5 end
  if type(overlap) ~= 'number' then error('cfg.box_voting.overlap is not a number') end
  if not (overlap > 0 and overlap <= 1) then error('cfg.box_voting.overlap must be in (0, 1]') end
  return overlap, weight
end

-- cfg.nms -> method, overlap, sigma, min_score (validated on the host, before any device call).  The setting governs the
-- per-class pass only (Detector.lua:125-136); the first NMS is untouched.
--   method     'hard' (default: the reference -- a box that overlaps a better one of its class by more than `overlap` is deleted),
--              'linear' (its confidence is multiplied by 1 - IoU instead) or 'gaussian' (every box of the class has its
--              confidence multiplied by exp(-IoU^2 / sigma)); a box is dropped when its confidence falls below min_score
--   overlap    Nt, in (0, 1]; default 0.1, the reference's threshold
--   sigma      > 0; default 0.5
--   min_score  in [0, 1), a probability; default 0.001; 0 keeps every class-test survivor
function Detector.nms_settings(t)
  if t == nil then t = {} end
  if type(t) ~= 'table' then error('cfg.nms must be a table of {method, overlap, sigma, min_score}') end
  for k, _ in pairs(t) do
    if k ~= 'method' and k ~= 'overlap' and k ~= 'sigma' and k ~= 'min_score' then
      error('cfg.nms: unknown key ' .. tostring(k))
    end
  end
  local method = t.method
  if method == nil then method = 'hard' end
  if method ~= 'hard' and method ~= 'linear' and method ~= 'gaussian' then
    error('cfg.nms.method must be "hard", "linear" or "gaussian"')
  end
  local function number(name, default)
    local v = t[name]
    if v == nil then return default end
    if type(v) ~= 'number' then error('cfg.nms.' .. name .. ' is not a number') end
    return v
  end
  local overlap, sigma, min_score = number('overlap', 0.1), number('sigma', 0.5), number('min_score', 0.001)
  if not (overlap > 0 and overlap <= 1) then error('cfg.nms.overlap must be in (0, 1]') end
  if not (sigma > 0 and sigma < math.huge) then error('cfg.nms.sigma must be > 0') end
  if not (min_score >= 0 and min_score < 1) then error('cfg.nms.min_score must be in [0, 1)') end
  return method, overlap, sigma, min_score
end

-- cfg.proposals -> order, pre_nms_top_n, post_nms_top_n (validated on the host, before any device call).
--   order           'y2' (default: the reference -- nms.lua ignores the scores it is handed, boxes go by descending max-y) or
--                   'score': the first NMS runs on rows {box, p} keyed by p (key_mode 2, key_col 5), the per-class NMS keyed by
--                   the confidence (key_col 5); the NMS tie rule is unchanged
--   pre_nms_top_n   nil or K >= 1: only the K' = min(n, K) best-ranked of a frame's n matches reach the first NMS.  Rank: the
--                   match's fp32 p compared as a value (-0 equals +0, a NaN ranks below everything), ties are broken by the
--                   lower scan row.  The selected rows keep their scan order, so K >= n changes nothing.  Either order.
--   post_nms_top_n  nil or M >= 1: the candidates are the first min(R, M) picks of the first NMS; needs order = 'score'
function Detector.proposal_settings(t)
  if t == nil then t = {} end
  if type(t) ~= 'table' then error('cfg.proposals must be a table of {order, pre_nms_top_n, post_nms_top_n}') end
  for k, _ in pairs(t) do
    if k ~= 'order' and k ~= 'pre_nms_top_n' and k ~= 'post_nms_top_n' then
      error('cfg.proposals: unknown key ' .. tostring(k))
    end
  end
  local order = t.order
  if order == nil then order = 'y2' end
  if order ~= 'y2' and order ~= 'score' then error('cfg.proposals.order must be "y2" or "score"') end
  local function top_n(name)
    local v = t[name]
    if v == nil then return nil end
    if type(v) ~= 'number' or v ~= math.floor(v) then error('cfg.proposals.' .. name .. ' is not an integer') end
    if v < 1 then error('cfg.proposals.' .. name .. ' must be at least 1') end
    return v
  end
  local pre, post = top_n('pre_nms_top_n'), top_n('post_nms_top_n')
  if post ~= nil and order ~= 'score' then
    error('cfg.proposals.post_nms_top_n needs order = "score": the first picks in max-y order are not the best')
  end
  return order, pre, post
end

-- pre_nms_top_n: the min(n_b, K) best-scoring rows of every frame's matches (B x cap rows, device counts cnt), gathered in
-- scan order into compact arrays of kcap = min(cap, K) rows per frame; count = the selected counts (device int[B])
function Detector:select_rows(mp, mi, mr, mb, B, cap, K, cnt, pre)
  local scratch = self.scratch
  local kcap = math.min(cap, K)
  local sel = ffi.cast('int*', scratch(pre .. 'sel', 4 * B * kcap).ptr)
  local kcnt = ffi.cast('int*', scratch(pre .. 'sel_count', 4 * B).ptr)
  local wsb = tonumber(C.frcnn_topk_select_workspace_bytes(B, cap))
  local ws = scratch(pre .. 'sel_ws', wsb)
  check(C.frcnn_topk_select(mp, B, cap, cap, cnt, K, sel, kcap, kcnt, ws.ptr, wsb, nil))
  local out = { count = kcnt, stride = kcap,
                p = ffi.cast('float*', scratch(pre .. 'sel_p', 4 * B * kcap).ptr),
                idx = ffi.cast('int*', scratch(pre .. 'sel_idx', 16 * B * kcap).ptr),
                rect = ffi.cast('double*', scratch(pre .. 'sel_rect', 32 * B * kcap).ptr),
                box = ffi.cast('float*', scratch(pre .. 'sel_box', 16 * B * kcap).ptr),
                box5 = ffi.cast('float*', scratch(pre .. 'sel_box5', 20 * B * kcap).ptr),
                row = ffi.cast('int*', scratch(pre .. 'sel_row', 4 * B * kcap).ptr) }
  check(C.frcnn_rpn_gather_rows(mp, mi, mr, mb, B, cap, cap, sel, kcap, kcnt, kcap, out.p, out.idx, out.rect, out.box, out.box5,
                                out.row, kcap, nil))
  return out
end

-- order = 'score' without a cap: rows {box, p} of every match (the count read on the device), the first NMS's input
function Detector:score_rows(mp, mb, B, cap, cnt, pre)
  local box5 = ffi.cast('float*', self.scratch(pre .. 'box5', 20 * B * cap).ptr)
  check(C.frcnn_rpn_gather_rows(mp, nil, nil, mb, B, cap, cap, nil, 0, cnt, cap, nil, nil, nil, nil, box5, nil, cap, nil))
  return box5
end

-- post_nms_top_n: the candidate counts clamped on the host; the device copy (what the winner table's header reports) follows
function Detector:clamp_candidates(dev, count, B)
  local changed = false
  for b = 0, B - 1 do
    if count[b] > self.post_nms_top_n then
      count[b] = self.post_nms_top_n
      changed = true
    end
  end
  if changed then check(C.frcnn_memcpy_h2d(dev, count, 4 * B, nil)) end
end

-- The ONE pipeline, for a chunk of B frames, of one size or not; Detector:detect(input) is the chunk { input }.
Detector.BATCH = 8              -- frames per chunk of detect_batch
Detector.NMS_FIRST_CAP = 16384  -- rows the first NMS launch is sized for (see first_stage)
Detector.CLASS_NMS_WORKSPACE = 2 * 2 ^ 30   -- bytes: under cfg.scoring a per-class NMS whose workspace would exceed them is refused

-- (h, w) of the output a Localizer's layer list yields for an H x W input: per layer ceil((n + 2 pad - k) / d) + 1, the native
-- model's arithmetic (stride-1 convolutions, ceil-mode 2x2 pooling)
local function map_hw(layers, H, W)
  local h, w = H, W
  for _, l in ipairs(layers) do
    h = math.ceil((h + 2 * l.padH - l.kH) / l.dH) + 1
    w = math.ceil((w + 2 * l.padW - l.kW) / l.dW) + 1
  end
  return h, w
end

-- What a frame of H x W occupies in a chunk, from the layer lists Localizer.lua walks -- host arithmetic only, no pass, worked
-- out once per size: hw (the four head maps' { h, w }), fshape ({ planes, fh, fw } of the last feature map), hoff (the 5-entry
-- prefix of the head maps' float counts, 18 planes each, every one rounded up to 64: where map i lies in the frame's slot,
-- hoff[5] what the frame needs of it), fslot (likewise, the feature map) and anchors (of the four maps)
function Detector:layout(H, W)
  self.layouts = self.layouts or {}
  local key = H .. 'x' .. W
  local t = self.layouts[key]
  if t == nil then
    local function ceil64(n) return math.floor((n + 63) / 64) * 64 end
    local children = self.model.pnet.outnode.children
    local planes = self.model.layers[#self.model.layers].filters
    t = { hw = {}, hoff = { 0 }, anchors = 0 }
    for i = 1, 4 do
      local h, w = map_hw(Localizer.new(children[i]).layers, H, W)
      t.hw[i] = { h, w }
      t.hoff[i + 1] = t.hoff[i] + ceil64(ASPECTS * 6 * h * w)
      t.anchors = t.anchors + ASPECTS * h * w
    end
    local fh, fw = map_hw(Localizer.new(children[self.nheads + 1]).layers, H, W)
    t.fshape, t.fslot = { planes, fh, fw }, ceil64(planes * fh * fw)
    self.layouts[key] = t
  end
  return t
end

-- Detector.lua:17-85 for a chunk: the proposal net frame by frame, ONE scan, (selection or score rows), ONE segmented first
-- NMS, read-back 1 of 2, alone again every frame over the bound, the post-NMS clamp -> a table { B, cnt (device int[4][B]),
-- cap (rows a frame in mp, mi, mr, dpick: the match arrays the rest of the chunk reads, the selected rows under
-- pre_nms_top_n), fm, fslot, fs (frame b's last feature map at fm + b * fslot, its size fs[b]), count (host int[2][B]: rows and
-- candidates per frame), key_mode, key_col (of both NMS passes) }.  prefix: of the scratch names ('' for detect and proposals,
-- 'b_' for detect_batch: neither overwrites what the other left behind)
function Detector:first_stage(frames, prefix)
  local pnet = self.model.pnet
  local scratch = self.scratch
  local B = #frames
  local nout = self.nheads + 1

  -- ---- 1. per frame: the proposal net; its head maps and last feature map are copied to the frame's slot (the net reuses its
  --         output buffers).  Where they lie follows from the frame's size on the host (layout, checked against what the net
  --         hands back), so the slots -- strided by the chunk's largest frame -- are sized before the first pass: frame b's four
  --         head maps lie packed at hoff[i] of slot b of `heads`, its last feature map at the start of slot b of `fm`.  A chunk
  --         of ONE frame reads the net's buffers where they are: no copies
  pnet:evaluate()                                                       -- :31
  -- counts (device int[4][B]): per frame matches, NMS candidates, candidates that pass the class test, winners
  local cnt = ffi.cast('int*', scratch(prefix .. 'counts', 16 * B).ptr)
  local size1 = frames[1]:size()
  local lay, fs, anchors, one_size = {}, {}, {}, true
  local slot, fslot, cap = 0, 0, 0
  for b = 0, B - 1 do
    local size = frames[b + 1]:size()
    if size[2] ~= size1[2] or size[3] ~= size1[3] then one_size = false end
    local t = self:layout(size[2], size[3])
    lay[b], fs[b], anchors[b] = t, t.fshape, t.anchors
    slot, fslot, cap = math.max(slot, t.hoff[5]), math.max(fslot, t.fslot), math.max(cap, t.anchors)
  end
  local maps, heads, fm = ffi.new('const float*[4]')
  if B > 1 then
    heads = ffi.cast('float*', scratch(prefix .. 'heads', 4 * B * slot).ptr)
    fm = ffi.cast('float*', scratch(prefix .. 'fm', 4 * B * fslot).ptr)
  end
  for b = 0, B - 1 do
    local t = lay[b]
    local outputs = pnet:forward(hip.to_device(frames[b + 1]))          -- :32-33
    for i = 1, nout do
      local s = outputs[i]:size()
      local want = t.fshape
      if i < nout then want = { ASPECTS * 6, t.hw[i][1], t.hw[i][2] } end
      if s[1] ~= want[1] or s[2] ~= want[2] or s[3] ~= want[3] then
        error(string.format('Detector: output %d of frame %d is %dx%dx%d, expected %dx%dx%d', i, b + 1, s[1], s[2], s[3],
                            want[1], want[2], want[3]))
      end
    end
    if B == 1 then
      for i = 1, 4 do maps[i - 1] = outputs[i].ptr end
      fm = ffi.cast('float*', outputs[nout].ptr)
    else
      for i = 1, 4 do
        check(C.frcnn_memcpy_d2d(heads + b * slot + t.hoff[i], outputs[i].ptr, 4 * ASPECTS * 6 * t.hw[i][1] * t.hw[i][2], nil))
      end
      check(C.frcnn_memcpy_d2d(fm + b * fslot, outputs[nout].ptr, 4 * t.fshape[1] * t.fshape[2] * t.fshape[3], nil))
    end
  end
  -- ---- 2. ONE scan over the B slots (:39-66 on the device: log-softmax of every anchor's two logits, p > 0.95, decode,
  --         overlap test, compaction): frame b's matches at rows [b * cap, b * cap + n_b).  Every anchor of the four maps may
  --         pass (vgg_large 1000x600: 45 015): the buffers hold them all; cap is the largest frame's anchor count.  A chunk of
  --         one size takes frcnn_rpn_scan_batch (the four maps of slot 0 -- or the net's own --, the slot stride, that size), a
  --         chunk that mixes sizes frcnn_rpn_scan_ragged (per-frame map sizes, offsets and image sizes): the same bodies, 3 %
  --         dearer a call
  local Hs, Ws = ffi.new('int[?]', 4 * B), ffi.new('int[?]', 4 * B)
  for b = 0, B - 1 do
    for i = 1, 4 do Hs[4 * b + i - 1], Ws[4 * b + i - 1] = lay[b].hw[i][1], lay[b].hw[i][2] end
  end
  local wsb
  if one_size then
    wsb = tonumber(C.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, B))
  else
    wsb = tonumber(C.frcnn_rpn_scan_ragged_workspace_bytes(Hs, Ws, B))
  end
  local ws = scratch(prefix .. 'scan_ws', wsb)
  local mp = ffi.cast('float*', scratch(prefix .. 'match_p', 4 * B * cap).ptr)
  local mi = ffi.cast('int*', scratch(prefix .. 'match_idx', 16 * B * cap).ptr)
  local mr = ffi.cast('double*', scratch(prefix .. 'match_rect', 32 * B * cap).ptr)
  local mb = ffi.cast('float*', scratch(prefix .. 'match_box', 16 * B * cap).ptr)
  if one_size then
    if B > 1 then
      for i = 0, 3 do maps[i] = heads + lay[0].hoff[i + 1] end
    end
    check(C.frcnn_rpn_scan_batch(maps, Hs, Ws, B, slot, self.aw.ptr, self.ah.ptr, size1[3], size1[2], 0.95, cap,
                                 mp, mi, mr, mb, cnt, ws.ptr, wsb, nil))
  else
    local map_off, img_wh = ffi.new('long long[?]', 4 * B), ffi.new('double[?]', 2 * B)
    for b = 0, B - 1 do
      local size = frames[b + 1]:size()
      img_wh[2 * b], img_wh[2 * b + 1] = size[3], size[2]
      for i = 1, 4 do map_off[4 * b + i - 1] = b * slot + lay[b].hoff[i] end
    end
    check(C.frcnn_rpn_scan_ragged(heads, map_off, Hs, Ws, img_wh, B, self.aw.ptr, self.ah.ptr, 0.95, cap, mp, mi, mr, mb, cnt,
                                  ws.ptr, wsb, nil))
  end
  -- ---- 3. ONE segmented NMS (:74-85) on the device, the match counts read from DEVICE memory (no round trip between scan
  --         and NMS); the score tensor is ignored by nms.lua -> key = max-y.  Launch and workspace are sized for a bound on
  --         the matches, not for every anchor of the maps; a frame with more matches repeats the pass alone, sized by the
  --         count just read.  Under pre_nms_top_n = K the match arrays are replaced by the compact arrays of the K
  --         best-scoring rows (`cap` rows a frame from here on: min(cap, K)), which no frame can exceed; order = 'score':
  --         rows {box, p} keyed by p
  local order, pre, post = self.proposal_order, self.pre_nms_top_n, self.post_nms_top_n
  local key_mode, key_col = 0, 0
  if order == 'score' then key_mode, key_col = 2, 5 end
  local ncap = math.min(cap, Detector.NMS_FIRST_CAP)
  local ndev, boxes, ncols = cnt, mb, 4
  if order == 'score' and pre == nil then boxes, ncols = self:score_rows(mp, mb, B, cap, cnt, prefix), 5 end
  if pre ~= nil then
    local sel = self:select_rows(mp, mi, mr, mb, B, cap, pre, cnt, prefix)
    mp, mi, mr, mb = sel.p, sel.idx, sel.rect, sel.box
    cap, ncap, ndev, boxes = sel.stride, sel.stride, sel.count, sel.box
    if order == 'score' then boxes, ncols = sel.box5, 5 end
  end
  local nwsb = tonumber(C.frcnn_nms_batch_workspace_bytes(B, ncap))
  local nws = scratch(prefix .. 'nms_ws', nwsb)
  local dpick = ffi.cast('long long*', scratch(prefix .. 'pick', 8 * B * cap).ptr)
  check(C.frcnn_nms_device_batch(boxes, B, cap, ncap, ndev, ncols, 0.25, key_mode, key_col, nil, dpick, cnt + B, nws.ptr, nwsb, nil))
  local count = ffi.new('int[?]', 2 * B)
  check(C.frcnn_memcpy_d2h(count, cnt, 8 * B, nil))                      -- ---- read-back 1 of 2: B pairs of counts
  check(C.frcnn_stream_sync(nil))
  for b = 0, B - 1 do
    if count[b] > anchors[b] then
      error(string.format('Detector: %d anchors pass p > 0.95, more than the %d the maps hold', count[b], anchors[b]))
    end
    if pre ~= nil then count[b] = math.min(count[b], pre) end           -- rows of the (compact) match arrays from here on
    if count[b] > ncap then
      local fwsb = tonumber(C.frcnn_nms_workspace_bytes(count[b]))
      local fws = scratch(prefix .. 'nms_ws_full', fwsb)
      check(C.frcnn_nms_device(boxes + ncols * b * cap, count[b], ncols, 0.25, key_mode, key_col, dpick + b * cap, cnt + B + b,
                               fws.ptr, fwsb, nil))
      check(C.frcnn_memcpy_d2h(count + B + b, cnt + B + b, 4, nil))
      check(C.frcnn_stream_sync(nil))
    end
  end
  if post ~= nil then self:clamp_candidates(cnt + B, count + B, B) end
  return { B = B, cnt = cnt, cap = cap, mp = mp, mi = mi, mr = mr, dpick = dpick, fm = fm, fslot = fslot, fs = fs, count = count,
           key_mode = key_mode, key_col = key_col }
end

-- Detector:proposals(input) -- the candidates of the first NMS (Detector.lua:17-85) without the classification net: a list of
-- { p, a, r, l } as in a detection, in pick order (under the proposal settings of this Detector)
function Detector:proposals(input)
  local st = self:first_stage({ input }, '')
  local list = {}
  local nm, R = st.count[0], st.count[1]
  if nm == 0 or R == 0 then return list end
  local hp, hi, hr = ffi.new('float[?]', nm), ffi.new('int[?]', 4 * nm), ffi.new('double[?]', 4 * nm)
  local hpick = ffi.new('long long[?]', R)
  check(C.frcnn_memcpy_d2h(hp, st.mp, 4 * nm, nil))
  check(C.frcnn_memcpy_d2h(hi, st.mi, 16 * nm, nil))
  check(C.frcnn_memcpy_d2h(hr, st.mr, 32 * nm, nil))
  check(C.frcnn_memcpy_d2h(hpick, st.dpick, 8 * R, nil))
  check(C.frcnn_stream_sync(nil))
  for q = 0, R - 1 do
    local i = tonumber(hpick[q]) - 1
    local l, a, y, x = hi[4 * i], hi[4 * i + 1], hi[4 * i + 2], hi[4 * i + 3]
    list[#list + 1] = { p = hp[i], a = self.anchors:get(l, a, y, x), l = l,
                        r = Rect.new(hr[4 * i], hr[4 * i + 1], hr[4 * i + 2], hr[4 * i + 3]) }
  end
  return list
end

function Detector:detect(input)                                         -- Detector.lua:17-141
  self:view_lists({ input:size() })                                     -- (cfg.tta: refused before anything is queued)
  return self:detect_chunk({ input }, false, '')[1]
end

-- Detector:detect_batch(inputs, opts) -- detect() for a list of frames -- of ONE size, or (opts.mixed_sizes) of any sizes: a list
-- with one entry per frame, in order, each what detect(frame) returns.  opts: a table { shared_cnet = bool, mixed_sizes = bool,
-- scoring = a table as Detector.scoring_settings takes it, tta = a table as Detector.tta_settings takes it }, or (as before) the
-- boolean shared_cnet itself.  Under cfg.tta a chunk holds max(1, floor(Detector.BATCH / V)) frames: its segments are their views.
-- Chunks of Detector.BATCH frames: the proposal net runs frame by frame (its
-- head maps and last feature map are copied to the frame's slot), then ONE scan, ONE segmented NMS, per frame with
-- candidates the pooling / classification net / class test, ONE segmented per-class NMS and ONE gather; the host waits
-- twice per chunk instead of twice per frame.  Bit-identical to detect() frame by frame: detect() is a chunk of one.
-- shared_cnet = true: ONE classification-net pass over the candidates of all frames of a chunk (frame b's rows at the prefix
-- sum of the candidate counts); everything up to the pooled rows stays bit-identical, the net's outputs agree with detect()'s
-- within the net's own error only (input scale and Linear form depend on the whole tensor / the row count).
-- mixed_sizes = false (default): frames of different sizes are refused before anything is queued.  true: the chunks are the
-- consecutive Detector.BATCH frames whatever their sizes.  Every chunk takes the one front of first_stage: each frame lies in
-- its slot by its own size's layout, the slots are strided by the chunk's largest frame, and ONE scan follows --
-- frcnn_rpn_scan_batch when the chunk has one size (then the strides are that size's own), else frcnn_rpn_scan_ragged with
-- per-frame map sizes and image sizes; everything behind the scan reads per-frame device counts already, so nothing else
-- changes and every frame's result stays what detect(frame) returns.
-- 1:1 with Detector.detect_batch of the Python host mirror.
function Detector:detect_batch(inputs, opts)
  local shared_cnet, mixed_sizes = opts, false
  if type(opts) == 'table' then
    shared_cnet, mixed_sizes = opts.shared_cnet, opts.mixed_sizes
    if opts.scoring ~= nil then self:set_scoring(opts.scoring) end     -- (validated before anything is queued; it stays set)
    if opts.tta ~= nil then self:set_tta(opts.tta) end                 -- (likewise)
  end
  local nframes = #inputs
  local function same_size(i, j)
    local a, b = inputs[i]:size(), inputs[j]:size()
    return a[1] == b[1] and a[2] == b[2] and a[3] == b[3]
  end
  for i = 1, nframes do                                                 -- refused before anything is queued
    if mixed_sizes then       -- (:dim() and indexing what :size() returns: both host and device tensors have them)
      if inputs[i]:dim() ~= 3 or inputs[i]:size()[1] ~= 3 then error('Detector:detect_batch: expected 3xHxW frames') end
    elseif not same_size(1, i) then
      error('Detector:detect_batch: frames of different sizes in one call')
    end
  end
  local sizes = {}
  for i = 1, nframes do sizes[i] = inputs[i]:size() end
  local step = Detector.BATCH
  local lists, V = self:view_lists(sizes)                               -- (cfg.tta: refused before anything is queued)
  if lists ~= nil then step = math.max(1, math.floor(step / V)) end     -- a chunk's segments are its frames' views
  local results = {}
  local lo = 1
  while lo <= nframes do
    local chunk = {}
    for i = lo, math.min(lo + step - 1, nframes) do chunk[#chunk + 1] = inputs[i] end
    for _, winners in ipairs(self:detect_chunk(chunk, shared_cnet, 'b_')) do results[#results + 1] = winners end
    lo = lo + step
  end
  return results
end

-- Detector:match_batch(inputs, ground_truth, opts) -- detect_batch(inputs) matched to the frames' ground truth ON THE DEVICE, for
-- mean average precision (not in the reference; include/frcnn_hip_eval.h).  ground_truth[f]: the frame's boxes, a list of
-- { class_index = c, rect = Rect } (what nextValidation hands out) or of { c, Rect }, at most 1024.  opts: detect_batch's table,
-- and iou_thresholds (default { 0.5 }, at most 16) and with_iou.  -> per frame { cls, confidence, tp, gt [, iou] }: arrays whose
-- entry k describes detect_batch(inputs)[f][k]; bit t of tp[k] (bit.band(tp[k], bit.lshift(1, t)) ~= 0) is a true positive at
-- threshold t + 1 of the list, gt[k] the 1-based box (0: none).  The pipeline is detect_batch's, unchanged, up to and including
-- the gather; behind it max_detections is applied by frcnn_eval_conf_rows + frcnn_topk_select, ONE frcnn_eval_match_batch matches
-- the chunk, and read-back 2 brings 16 bytes a row in place of the 128-byte records.  Under cfg.tta: one result per original
-- frame.  1:1 with Detector.match_batch of the Python host mirror.
Detector.MATCH_MAX_THRESHOLDS, Detector.MATCH_MAX_BOXES = 16, 1024
function Detector:match_batch(inputs, ground_truth, opts)
  opts = opts or {}
  local thr = opts.iou_thresholds or { 0.5 }
  if #thr < 1 or #thr > Detector.MATCH_MAX_THRESHOLDS then error('Detector:match_batch: 1 ... 16 IoU thresholds') end
  for _, t in ipairs(thr) do if type(t) ~= 'number' or t ~= t then error('Detector:match_batch: a threshold is not a number') end end
  if #ground_truth ~= #inputs then error('Detector:match_batch: ground truth for ' .. #ground_truth .. ' of ' .. #inputs .. ' frames') end
  local gts = {}
  for f, boxes in ipairs(ground_truth) do
    if #boxes > Detector.MATCH_MAX_BOXES then error('Detector:match_batch: more than 1024 ground-truth boxes in a frame') end
    local g = { cls = {}, rect = {} }
    for i, x in ipairs(boxes) do
      local r = x.rect or x[2]
      g.cls[i], g.rect[i] = x.class_index or x[1], { r.minX, r.minY, r.maxX, r.maxY }
    end
    gts[f] = g
  end
  if opts.scoring ~= nil then self:set_scoring(opts.scoring) end
  if opts.tta ~= nil then self:set_tta(opts.tta) end
  local nframes, sizes = #inputs, {}
  for i = 1, nframes do
    sizes[i] = inputs[i]:size()
    if inputs[i]:dim() ~= 3 or sizes[i][1] ~= 3 then error('Detector:match_batch: expected 3xHxW frames') end
    if not opts.mixed_sizes and (sizes[i][2] ~= sizes[1][2] or sizes[i][3] ~= sizes[1][3]) then
      error('Detector:match_batch: frames of different sizes in one call')
    end
  end
  local step = Detector.BATCH
  local lists, V = self:view_lists(sizes)
  if lists ~= nil then step = math.max(1, math.floor(step / V)) end
  local results = {}
  local lo = 1
  while lo <= nframes do
    local chunk, gt = {}, {}
    for i = lo, math.min(lo + step - 1, nframes) do chunk[#chunk + 1], gt[#gt + 1] = inputs[i], gts[i] end
    local m = { gt = gt, thr = thr, with_iou = opts.with_iou and true or false }
    for _, r in ipairs(self:detect_chunk(chunk, opts.shared_cnet, 'b_', m)) do results[#results + 1] = r end
    lo = lo + step
  end
  return results
end

-- The chunk's winner tables `out` (just queued) against match.gt: the ground truth's upload, under max_detections
-- frcnn_eval_conf_rows + frcnn_topk_select (the rank of the host's sort: fp32 values, ties to the earlier pick), ONE
-- frcnn_eval_match_batch, then read-back 2 of 2 -- the match tables and, asked for, the overlaps, in ONE copy and wait
function Detector:match_tables(match, out, B, rows, prefix)
  local scratch, CE = self.scratch, hip.CE
  local row0 = ffi.new('long long[?]', B + 1)
  local G = 0
  for b = 1, B do
    row0[b - 1] = G
    G = G + #match.gt[b].cls
  end
  row0[B] = G
  local hrect, hcls = ffi.new('double[?]', 4 * math.max(G, 1)), ffi.new('int[?]', math.max(G, 1))
  local g = 0
  for b = 1, B do
    for i, c in ipairs(match.gt[b].cls) do
      hcls[g] = c
      for t = 1, 4 do hrect[4 * g + t - 1] = match.gt[b].rect[i][t] end
      g = g + 1
    end
  end
  local drect = ffi.cast('double*', scratch(prefix .. 'gt_rect', 32 * math.max(G, 1)).ptr)
  local dcls = ffi.cast('int*', scratch(prefix .. 'gt_class', 4 * math.max(G, 1)).ptr)
  if G > 0 then
    check(C.frcnn_memcpy_h2d(drect, hrect, 32 * G, nil))
    check(C.frcnn_memcpy_h2d(dcls, hcls, 4 * G, nil))
  end
  local sel, kcap, kd = nil, 0, nil
  if self.max_detections ~= nil and rows > 0 then
    kcap = math.min(rows, self.max_detections)
    local conf = ffi.cast('float*', scratch(prefix .. 'eval_conf', 4 * B * rows).ptr)
    local wcnt = ffi.cast('int*', scratch(prefix .. 'eval_count', 4 * B).ptr)
    sel = ffi.cast('int*', scratch(prefix .. 'eval_sel', 4 * B * kcap).ptr)
    kd = ffi.cast('int*', scratch(prefix .. 'eval_k', 4 * B).ptr)
    local wsb = tonumber(C.frcnn_topk_select_workspace_bytes(B, rows))
    local ws = scratch(prefix .. 'eval_sel_ws', wsb)
    check(CE.frcnn_eval_conf_rows(out, B, rows, conf, wcnt, nil))
    check(C.frcnn_topk_select(conf, B, rows, rows, wcnt, self.max_detections, sel, kcap, kd, ws.ptr, wsb, nil))
  end
  local T = #match.thr
  local thr = ffi.new('double[?]', T)
  for t = 1, T do thr[t - 1] = match.thr[t] end
  local tbytes = 16 * B * (rows + 2)
  local nbytes = tbytes + (match.with_iou and 8 * B * rows or 0)
  local dev = ffi.cast('char*', scratch(prefix .. 'eval_match', nbytes).ptr)
  local diou = nil
  if match.with_iou then diou = ffi.cast('double*', dev + tbytes) end
  check(CE.frcnn_eval_match_batch(out, B, rows, sel, kcap, kd, drect, dcls, row0, thr, T, ffi.cast('int*', dev), diou, nil))
  local h = ffi.new('char[?]', nbytes)
  check(C.frcnn_memcpy_d2h(h, dev, nbytes, nil))                          -- ---- read-back 2 of 2: 16 bytes a row
  check(C.frcnn_stream_sync(nil))
  local tabs, ious = ffi.cast('int*', h), ffi.cast('double*', h + tbytes)
  local results = {}
  for b = 0, B - 1 do
    local tab = tabs + 4 * b * (rows + 2)
    local n = tab[4]
    -- classes in ascending order, the table's order within a class: the order of detect_batch's list
    local order = {}
    for q = 1, n do order[q] = q end
    table.sort(order, function(i, j)
      local ci, cj = tab[4 * (i + 1)], tab[4 * (j + 1)]
      if ci ~= cj then return ci < cj end
      return i < j
    end)
    local r = { cls = {}, confidence = {}, tp = {}, gt = {}, iou = match.with_iou and {} or nil }
    for k, q in ipairs(order) do
      local v = tab + 4 * (q + 1)
      r.cls[k], r.tp[k], r.gt[k] = v[0], v[2], v[3]
      r.confidence[k] = tonumber(ffi.cast('float*', v + 1)[0])
      if match.with_iou then r.iou[k] = ious[b * rows + q - 1] end
    end
    results[b + 1] = r
  end
  return results
end

-- Detector.average_precision_from_matches(matches, ground_truth, thresholds, use_07_metric) -- AP per class and mAP from what
-- match_batch returns (the matching is done: per class the stable sort by decreasing confidence across the frames, the
-- cumulative sums, the area under the monotone precision envelope or the 11-point average).  thresholds: the list match_batch
-- was called with -> { mAP, by_iou = { [t] = { mAP, ap, npos, tp, fp } } }.  1:1 with evaluation.average_precision_from_matches.
function Detector.average_precision_from_matches(matches, ground_truth, thresholds, use_07_metric)
  local npos, classes = {}, {}
  for _, boxes in ipairs(ground_truth) do
    for _, x in ipairs(boxes) do
      local c = x.class_index or x[1]
      if npos[c] == nil then
        npos[c] = 0
        classes[#classes + 1] = c
      end
      npos[c] = npos[c] + 1
    end
  end
  table.sort(classes)
  local by_iou, sum = {}, 0
  for ti, t in ipairs(thresholds) do
    local res = { ap = {}, npos = npos, tp = 0, fp = 0 }
    local total = 0
    for _, c in ipairs(classes) do
      local dets = {}
      for f, m in ipairs(matches) do
        for k = 1, #m.cls do
          if m.cls[k] == c then dets[#dets + 1] = { m.confidence[k], #dets + 1, bit.band(m.tp[k], bit.lshift(1, ti - 1)) ~= 0 } end
        end
      end
      table.sort(dets, function(a, b)
        if a[1] ~= b[1] then return a[1] > b[1] end
        return a[2] < b[2]
      end)
      local rec, prec, ctp = {}, {}, 0
      for k, d in ipairs(dets) do
        if d[3] then ctp = ctp + 1 end
        rec[k], prec[k] = ctp / npos[c], ctp / k
      end
      res.tp, res.fp = res.tp + ctp, res.fp + #dets - ctp
      local ap = 0
      if use_07_metric then
        for i = 0, 10 do
          local p = 0
          for k = 1, #dets do if rec[k] >= i / 10 and prec[k] > p then p = prec[k] end end
          ap = ap + p / 11
        end
      else
        for k = #dets - 1, 1, -1 do prec[k] = math.max(prec[k], prec[k + 1]) end
        local last = 0
        for k = 1, #dets do
          ap = ap + (rec[k] - last) * prec[k]
          last = rec[k]
        end
      end
      res.ap[c] = ap
      total = total + ap
    end
    res.mAP = #classes > 0 and total / #classes or 0 / 0
    by_iou[t] = res
    sum = sum + res.mAP
  end
  return { mAP = sum / #thresholds, by_iou = by_iou }
end

-- Detector:evaluate_detections(frames, ground_truth, opts) -- mean average precision of this Detector on frames with their
-- ground truth (evaluation.evaluate_detections of the Python mirror on frames already loaded).  opts.match = 'host' (default): the
-- lists of detect_batch are matched here, detection by detection (the greedy loop: by decreasing confidence, a box is used by the
-- first that reaches it); 'device': match_batch.  The same table either way; anything else is refused before the device is touched.
function Detector:evaluate_detections(frames, ground_truth, opts)
  opts = opts or {}
  local how = opts.match or 'host'
  if how ~= 'host' and how ~= 'device' then error("Detector:evaluate_detections: match must be 'host' or 'device'") end
  local thr = opts.iou_thresholds or { 0.5 }
  local matches
  if how == 'device' then
    matches = self:match_batch(frames, ground_truth, opts)
  else
    matches = {}
    for f, winners in ipairs(self:detect_batch(frames, opts)) do
      local m = { cls = {}, confidence = {}, tp = {}, gt = {} }
      local order = {}
      for k, w in ipairs(winners) do
        m.cls[k], m.confidence[k], m.tp[k], m.gt[k] = w.class, tonumber(ffi.cast('float', w.confidence)), 0, 0
        order[k] = k
        local best = -1
        for j, x in ipairs(ground_truth[f]) do
          if (x.class_index or x[1]) == w.class then
            local v = Rect.IoU(w.r2, x.rect or x[2])
            if v > best then best, m.gt[k] = v, j end
          end
        end
        w.best = best
      end
      table.sort(order, function(i, j)
        if m.confidence[i] ~= m.confidence[j] then return m.confidence[i] > m.confidence[j] end
        return i < j
      end)
      for ti, t in ipairs(thr) do
        local used = {}
        for _, k in ipairs(order) do
          if m.gt[k] > 0 and winners[k].best >= t and not used[m.gt[k]] then
            used[m.gt[k]] = true
            m.tp[k] = bit.bor(m.tp[k], bit.lshift(1, ti - 1))
          end
        end
      end
      matches[f] = m
    end
  end
  return Detector.average_precision_from_matches(matches, ground_truth, thr, opts.use_07_metric)
end

-- detect() of a chunk of frames -> one list of winners per frame: first_stage, then -- unless no frame has a match -- per
-- frame the pooling, the classification net and the class test, ONE segmented per-class NMS, ONE gather, read-back 2 of 2.
-- Under cfg.tta the SEGMENTS of the chunk are the frames' views (frame f's V views at segments f * V ... f * V + V - 1):
-- first_stage and step 4 run on them as on frames, ONE frcnn_detect_merge_views launch then makes one segment per frame of them,
-- and step 5 runs on those -- B / V frames, V times the rows
-- match (Detector:match_batch; nil: nothing below is launched, allocated or read differently): { gt, thr, with_iou } -- behind
-- the gather the winners are matched to the ground truth on the device (match_tables), and a frame's result is its match arrays
function Detector:detect_chunk(frames, shared, prefix, match)
  local model = self.model
  local cfg = model.cfg
  local cnet = model.cnet
  local kh, kw, method, sampling = hip.roi_pooling_settings(cfg)
  local inv_sx, inv_sy = 0, 0                        -- RoIAlign reads the rects and the picks as they are: no window kernel
  if method == 'align' then inv_sx, inv_sy = hip.align_geometry(self.localizer) end
  local bgclass = cfg.class_count + 1
  local ncls = cfg.class_count + 1
  local D = kh * kw * model.layers[#model.layers].filters
  local scratch = self.scratch

  local sizes = {}
  for f, x in ipairs(frames) do sizes[f] = x:size() end
  local lists, V = self:view_lists(sizes)
  if lists ~= nil then
    local views = {}
    for f, x in ipairs(frames) do self:make_views(x, lists[f], f - 1, prefix, views) end
    frames = views
  end
  local st = self:first_stage(frames, prefix)                           -- :17-85
  local B, cnt, cap, mp, mi, mr, dpick, count = st.B, st.cnt, st.cap, st.mp, st.mi, st.mr, st.dpick, st.count
  local fm, fslot, key_mode, key_col = st.fm, st.fslot, st.key_mode, st.key_col
  local Rmax = 0
  for b = 0, B - 1 do
    if count[b] > 0 then Rmax = math.max(Rmax, count[B + b]) end
  end
  local results = {}
  for b = 1, (lists ~= nil) and B / V or B do
    results[b] = {}
    if match ~= nil then results[b] = { cls = {}, confidence = {}, tp = {}, gt = {}, iou = match.with_iou and {} or nil } end
  end
  if Rmax == 0 then return results end                                  -- :71, every frame
  -- ---- 4. per frame with candidates: REGION CLASSIFICATION (:90-101) and the class test (:106-122) into its segment
  --         (the net owns its outputs and reuses them, so a frame's class test follows its pass at once; the Python mirror, whose
  --         net writes into the frame's own rows, queues the passes of all frames first: per frame the same launches in the same
  --         order, and for one frame the same order altogether)
  cnet:evaluate()
  local nl = #self.localizer.layers
  local layers = ffi.new('int[?]', 6 * nl)
  for i, l in ipairs(self.localizer.layers) do
    local o = 6 * (i - 1)
    layers[o], layers[o + 1], layers[o + 2], layers[o + 3], layers[o + 4], layers[o + 5] = l.kW, l.kH, l.dW, l.dH, l.padW, l.padH
  end
  local dwins = ffi.cast('int*', scratch('wins', 16 * Rmax).ptr)
  local dcls = ffi.cast('int*', scratch(prefix .. 'cls', 4 * Rmax).ptr)
  local dconf = ffi.cast('float*', scratch(prefix .. 'conf', 4 * Rmax).ptr)
  -- Under cfg.scoring the class test is ONE frcnn_detect_classes_batch launch behind the passes of all frames, which reads the
  -- net's log-probabilities itself; 'all': a row per foreground class over min_confidence, so the per-row buffers and everything
  -- behind hold `rows` = Rmax * m a frame
  local scoring = self.scoring_classes ~= nil
  local rows = Rmax
  if scoring then rows = Rmax * self:scoring_rows(ncls) end
  local dbb = ffi.cast('float*', scratch(prefix .. 'bb5', 20 * B * rows).ptr)
  local dkc = ffi.cast('int*', scratch(prefix .. 'bbcls', 4 * B * rows).ptr)
  local dkeep = ffi.cast('int*', scratch(prefix .. 'keep_row', 4 * B * rows).ptr)
  local dr2 = ffi.cast('double*', scratch(prefix .. 'r2', 32 * B * rows).ptr)
  -- first row of frame b in the shared pass's input / output: the prefix sum of the candidate counts
  local row0, total = {}, 0
  for b = 0, B - 1 do
    if count[b] > 0 then
      row0[b] = total
      total = total + count[B + b]
    end
  end
  local cbuf = ffi.cast('float*', scratch(prefix .. 'cinput', 4 * (shared and total or Rmax) * D).ptr)
  -- the region features of frame b -> its input rows: every candidate's window (objective.lua:5-13 for all of them in one
  -- kernel) and one pooling launch (no indices: there is no backward pass), or one RoIAlign launch
  local function pooled(b)
    local R = count[B + b]
    local fs = st.fs[b]                                                 -- (the frame's own feature-map size)
    local cinput = hip.view(shared and (cbuf + row0[b] * D) or cbuf, { R, D })
    if method == 'align' then
      check(C.frcnn_roi_align_forward(fm + b * fslot, fs[1], fs[2], fs[3], mr + 4 * b * cap, dpick + b * cap, R, inv_sx, inv_sy,
                                      kh, kw, sampling, cinput.ptr, nil))
    else
      check(C.frcnn_roi_windows(mr + 4 * b * cap, dpick + b * cap, R, layers, nl, fs[2], fs[3], dwins, nil))
      check(C.frcnn_roi_pool_forward(fm + b * fslot, fs[1], fs[2], fs[3], dwins, R, kh, kw, cinput.ptr, nil, nil))
    end
    return cinput
  end
  -- cfg.scoring.boxes = 'class' under 'all': the box head's input of every pass is kept, in the rows of all_bbox / all_cls, for
  -- the class-row launch behind the class test
  local class_boxes = scoring and self.scoring_classes == 'all' and self.scoring_box == 'class'
  local nf, all_feat = cnet.feature_count, nil
  if class_boxes then
    all_feat = ffi.cast('float*', scratch(prefix .. 'feat', 4 * nf * (shared and total or B * Rmax)).ptr)
  end
  local all_bbox, all_cls
  if shared then
    for b = 0, B - 1 do
      if count[b] > 0 then pooled(b) end
    end
    local coutputs = cnet:forward(hip.view(cbuf, { total, D }))         -- :101, all frames
    all_bbox, all_cls = ffi.cast('float*', coutputs[1].ptr), ffi.cast('float*', coutputs[2].ptr)
    if class_boxes then cnet:features(all_feat) end
  elseif scoring then      -- the net reuses its outputs: every frame's are copied to its rows (b * Rmax) for the one launch
    all_bbox = ffi.cast('float*', scratch(prefix .. 'bbox', 16 * B * Rmax).ptr)
    all_cls = ffi.cast('float*', scratch(prefix .. 'cls_out', 4 * ncls * B * Rmax).ptr)
  end
  local R_arg, row0_arg = ffi.new('int[?]', B), ffi.new('long long[?]', B)     -- (zeroed: a frame without matches has no rows)
  for b = 0, B - 1 do
    local R = count[B + b]
    if count[b] > 0 then
      print(string.format('candidates: %d', R))                         -- :87
      local bbox_ptr, cls_ptr
      if shared then
        bbox_ptr, cls_ptr = all_bbox + 4 * row0[b], all_cls + ncls * row0[b]
        R_arg[b], row0_arg[b] = R, row0[b]
      else
        local coutputs = cnet:forward(pooled(b))                        -- :101
        bbox_ptr, cls_ptr = coutputs[1].ptr, coutputs[2].ptr
        if scoring then
          check(C.frcnn_memcpy_d2d(all_bbox + 4 * b * Rmax, bbox_ptr, 16 * R, nil))
          check(C.frcnn_memcpy_d2d(all_cls + ncls * b * Rmax, cls_ptr, 4 * ncls * R, nil))
          R_arg[b], row0_arg[b] = R, b * Rmax
          if class_boxes then cnet:features(all_feat + nf * b * Rmax) end
        end
      end
      if not scoring then
        check(C.frcnn_cnet_decode(cls_ptr, R, ncls, dcls, dconf, nil))  -- :110-113 (arg-max of the log-probs)
        -- :106-122 on the device: class test, r2 = Anchors.anchorToInput(r, bbox) in double, survivors compacted in order
        check(C.frcnn_detect_post(dcls, dconf, bbox_ptr, mr + 4 * b * cap, dpick + b * cap, R, bgclass, 0.2,
                                  dbb + 5 * b * Rmax, dkc + b * Rmax, dkeep + b * Rmax, dr2 + 4 * b * Rmax, cnt + 2 * B + b, nil))
      end
    elseif not scoring then
      check(C.frcnn_zero(cnt + 2 * B + b, 4, nil))                      -- no candidates: an empty segment of the per-class NMS
    end
  end
  if scoring then
    local mode = 0
    if self.scoring_classes == 'all' then mode = 1 end
    check(C.frcnn_detect_classes_batch(all_cls, all_bbox, R_arg, row0_arg, B, mr, dpick, cap, ncls, bgclass, self.min_confidence, mode,
                                       dbb, dkc, dkeep, dr2, rows, cnt + 2 * B, nil, nil))
    if class_boxes then
      -- ONE launch: row (r, c) gets the box class c's regressor rows predict for candidate r (the one written above was a
      -- placeholder); the row counts stay on the device.  In front of the merge of cfg.tta, which transforms these boxes too
      local W_box, b_box = hip.box_head_parameters(self.model)
      check(hip.CX.frcnn_detect_class_boxes_batch(all_feat, nf, row0_arg, B, W_box, b_box, ncls - 1, mr, dpick, cap, dkc, dkeep,
                                                  cnt + 2 * B, rows, dbb, dr2, nil))
    end
  end
  --         Under cfg.tta: ONE frcnn_detect_merge_views launch -- every frame's V segments of survivors become one segment of
  --         V * rows rows in the frame's coordinates (a view's geometry and its candidate count are host values since read-back 1:
  --         kernel arguments), the views' picks one pick list over the frame's V * cap match rows.  From here on the chunk has
  --         B / V segments; the match arrays are read where they lie
  local roff = nil
  if lists ~= nil then
    local S = B
    B = S / V
    local flip, wv, ax, ay = ffi.new('int[?]', S), ffi.new('double[?]', S), ffi.new('double[?]', S), ffi.new('double[?]', S)
    local R_seg = ffi.new('int[?]', S)
    roff = {}
    for f = 0, B - 1 do
      roff[f] = { 0 }
      for v = 0, V - 1 do
        local i, view = f * V + v, lists[f + 1][v + 1]
        flip[i], wv[i] = view[2] and 1 or 0, view[4]
        ax[i], ay[i] = sizes[f + 1][3] / view[4], sizes[f + 1][2] / view[3]
        if count[i] > 0 then R_seg[i] = count[S + i] end
        roff[f][v + 2] = roff[f][v + 1] + R_seg[i]
      end
    end
    local mbb = ffi.cast('float*', scratch(prefix .. 'tta_bb', 20 * S * rows).ptr)
    local mkc = ffi.cast('int*', scratch(prefix .. 'tta_kc', 4 * S * rows).ptr)
    local mkeep = ffi.cast('int*', scratch(prefix .. 'tta_keep_row', 4 * S * rows).ptr)
    local mr2 = ffi.cast('double*', scratch(prefix .. 'tta_r2', 32 * S * rows).ptr)
    local mpick = ffi.cast('long long*', scratch(prefix .. 'tta_pick', 8 * S * cap).ptr)
    local mcnt = ffi.cast('int*', scratch(prefix .. 'tta_counts', 16 * B).ptr)
    check(C.frcnn_detect_merge_views(dbb, dkc, dkeep, dr2, rows, cnt, dpick, cap, B, V, flip, wv, ax, ay, R_seg,
                                     mbb, mkc, mkeep, mr2, mpick, mcnt, nil))
    dbb, dkc, dkeep, dr2, dpick, cnt = mbb, mkc, mkeep, mr2, mpick, mcnt
    rows, cap = V * rows, V * cap
  end
  -- ---- 5. ONE segmented per-class NMS (:125-136; one segment per frame), every class in ONE device pass: rows only suppress
  --         rows of their own class; a stable partition of the picks by class is, per class, exactly nms(bb, 0.1, bb[{{}, 5}])
  --         -- the score tensor is ignored by nms.lua:42, the key is max-y (order = 'score': column 5, the confidence).  The
  --         survivor counts are read from device memory.  ONE gather of every frame's winner records (16 doubles each) behind
  --         a 128-byte header of the frame's four counts
  --         Under a soft method (cfg.nms): ONE frcnn_soft_nms_batch launch instead, on the log-confidences (log_domain 1,
  --         min_score as a log), which writes every winner's decayed score into column 5 of a COPY of bb; the gather reads that
  --         copy, so a winner's confidence is the score it was picked at
  local cpick = ffi.cast('long long*', scratch(prefix .. 'wpick', 8 * B * rows).ptr)
  local dbb_win = dbb
  -- (a frame's rows are its candidates times m: fewer candidates are the way out of either refusal)
  local remedy = ''
  if rows > Rmax then
    remedy = string.format(' (%d candidates x %d rows each: lower cfg.proposals.post_nms_top_n)', Rmax, rows / Rmax)
  end
  if self.nms_method ~= 'hard' then
    if rows > 16384 then
      error('Detector: more candidates in a frame than the 16384 a soft per-class NMS takes' .. remedy)
    end
    dbb_win = ffi.cast('float*', scratch(prefix .. 'bb_soft', 20 * B * rows).ptr)
    check(C.frcnn_memcpy_d2d(dbb_win, dbb, 20 * B * rows, nil))
    local swsb = tonumber(C.frcnn_soft_nms_workspace_bytes(B, rows))
    local sws = scratch(prefix .. 'soft_nms_ws', swsb)
    local log_min = -math.huge
    if self.nms_min_score > 0 then log_min = math.log(self.nms_min_score) end
    local method = 2
    if self.nms_method == 'linear' then method = 1 end
    check(C.frcnn_soft_nms_batch(dbb, B, rows, rows, cnt + 2 * B, 5, 5, method, self.nms_overlap, self.nms_sigma, log_min, 1, dkc,
                                 cpick, cnt + 3 * B, dbb_win + 4, 5, sws.ptr, swsb, nil))
  else
    local cwsb = tonumber(C.frcnn_nms_batch_workspace_bytes(B, rows))
    if scoring and cwsb > Detector.CLASS_NMS_WORKSPACE then
      error(string.format('Detector: the per-class NMS of %d frames of %d rows needs a workspace of %d bytes, more than the %d allowed',
                          B, rows, cwsb, Detector.CLASS_NMS_WORKSPACE) .. remedy)
    end
    local cws = scratch(prefix .. 'nms_ws2', cwsb)
    check(C.frcnn_nms_device_batch(dbb, B, rows, rows, cnt + 2 * B, 5, self.nms_overlap, key_mode, key_col, dkc, cpick, cnt + 3 * B,
                                   cws.ptr, cwsb, nil))
  end
  --         Under box voting (cfg.box_voting): ONE frcnn_box_vote_batch launch over the class test's survivors -- rows bb (the
  --         UNDECAYED log-confidences, also under a soft method: weight_mode 2), classes, coordinates the fp64 r2, winners cpick
  --         with the device winner counts -- writes the winners' voted rects into a buffer of their own, which the gather reads
  --         in place of r2
  local dr2_win = dr2
  if self.vote_overlap ~= nil then
    dr2_win = ffi.cast('double*', scratch(prefix .. 'r2_voted', 32 * B * rows).ptr)
    local weight_mode = 2
    if self.vote_weight == 'uniform' then weight_mode = 0 end
    check(C.frcnn_box_vote_batch(dbb, B, rows, rows, cnt + 2 * B, 5, 5, weight_mode, self.vote_overlap, dkc, dr2, cpick, cnt + 3 * B,
                                 dr2_win, nil, nil))
  end
  local out = ffi.cast('double*', scratch(prefix .. 'winners', 128 * B * (rows + 1)).ptr)
  check(C.frcnn_detect_gather_batch(cpick, cnt, B, rows, dkeep, dkc, dbb_win, dr2_win, dpick, cap, mp, mr, mi, out, nil))
  if match ~= nil then return self:match_tables(match, out, B, rows, prefix) end   -- match_batch: read-back 2 is the match tables
  local h = ffi.new('double[?]', 16 * B * (rows + 1))
  check(C.frcnn_memcpy_d2h(h, out, 128 * B * (rows + 1), nil))           -- ---- read-back 2 of 2: every frame's winner table
  check(C.frcnn_stream_sync(nil))
  for b = 0, B - 1 do
    local tab = h + 16 * b * (rows + 1)
    local nwin = ffi.cast('int*', tab)[3]
    -- classes in ascending order (the reference iterates with pairs(): unspecified), pick order within a class
    local byclass, classes = {}, {}
    -- max_detections: the M winners of highest confidence (compared as fp32 values, ties to the earlier pick), still in pick order
    local kept = nil
    if self.max_detections ~= nil and nwin > self.max_detections then
      local order = {}
      for q = 1, nwin do order[q] = q end
      local function conf(q) return tonumber(ffi.cast('float', tab[16 * q + 2])) end
      table.sort(order, function(i, j)
        if conf(i) ~= conf(j) then return conf(i) > conf(j) end
        return i < j
      end)
      kept = {}
      for i = 1, self.max_detections do kept[order[i]] = true end
    end
    for q = 1, nwin do if kept == nil or kept[q] then
      local v = tab + 16 * q
      local l, a, y, x = tonumber(v[12]), tonumber(v[13]), tonumber(v[14]), tonumber(v[15])
      local det = { p = v[3], a = self.anchors:get(l, a, y, x), l = l, r = Rect.new(v[4], v[5], v[6], v[7]),
                    r2 = Rect.new(v[8], v[9], v[10], v[11]), class = tonumber(v[0]), confidence = v[2] }
      if roff ~= nil then          -- the 0-based view the candidate came from: v[1] counts through the views' candidates
        det.candidate, det.view = tonumber(v[1]), 0
        while det.view + 1 < V and det.candidate > roff[b][det.view + 2] do det.view = det.view + 1 end
      end
      if not byclass[det.class] then
        byclass[det.class] = {}
        classes[#classes + 1] = det.class
      end
      table.insert(byclass[det.class], det)
    end end
    table.sort(classes)
    for _, ci in ipairs(classes) do
      for _, x in ipairs(byclass[ci]) do table.insert(results[b + 1], x) end
    end
  end
  return results
end
