-- nms.lua -- main.lua:7 / Detector.lua:3 `require 'nms'`: the global nms(boxes, overlap, scores) of the reference's nms.lua
-- (same dispatch on `scores`, same 1-based LongTensor result) served by frcnn_nms_host.  Found in place of the reference's
-- file when bindings/ precedes it on package.path.  soft_nms(boxes, overlap, score_col, ...) is not in the reference: Soft-NMS
-- on the device (frcnn_soft_nms_batch); nor is box_vote(boxes, picks, overlap, ...): bounding-box voting (frcnn_box_vote_batch).
local hip = require 'frcnn_hip'
nms = hip.nms
soft_nms = hip.soft_nms
box_vote = hip.box_vote
return nms
