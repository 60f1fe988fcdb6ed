"""faster-rcnn.torch_amd -- MI355X-native Faster R-CNN detection/training hot path behind the
reference's own surface (Rect, Localizer, Anchors, nms, Detector, create_objective, model factories).
All arithmetic runs in libfrcnn_hip.so (hand-written HIP for gfx950, C ABI in include/frcnn_hip.h);
this package is the host-side mirror of the Lua interface.  There is no CPU fallback."""
from . import _lib
from ._lib import FrcnnError
from .Anchors import Anchors, MT19937, manualSeed
from .BatchIterator import BatchIterator, decode_image, find_target_size, gaussian1D
from . import comm
from .comm import Comm
from .config import duplo_cfg, imgnet_cfg
from .Detector import Detector, scoring_boxes
from . import evaluation
from .evaluation import average_precision_from_matches, evaluate_detections, mean_average_precision, mean_average_precision_range, proposal_recall, validation_losses
from .Localizer import Localizer
from .model_utilities import create_model
from .nms import box_head, box_vote, class_boxes, cnet_loss, eval_match, nms, proposal_targets, roi_hard_select, soft_nms
from .objective import allreduce_begin, allreduce_begin_rest, allreduce_gradient_and_stats, box_head_settings, cnet_loss_settings, create_objective, extract_roi_pooling_input, roi_pooling_settings, roi_sampling_settings, roi_window, roi_windows
from .Rect import Rect
from . import t7, traindata
from .t7 import load_obj, restore_weights, save_model, save_obj
from .synthetic import Roi, SyntheticBatchIterator, assemble_examples, clean_examples, output_map_sizes, synthetic_image, synthetic_rois
from .tensor import DeviceTensor, ptr, stream_ptr, to_device
from .utilities import adam, combine_and_flatten_parameters, nag, optimizer, rmsprop, sgd
from .vgg_large import vgg_large
from .vgg_small import vgg_small

__all__ = ["Comm", "comm", "evaluation", "evaluate_detections", "mean_average_precision", "mean_average_precision_range", "proposal_recall", "validation_losses", "decode_image", "traindata", "t7", "load_obj", "restore_weights", "save_model", "save_obj", "BatchIterator", "find_target_size", "gaussian1D", "allreduce_begin", "allreduce_begin_rest", "Anchors", "Detector", "DeviceTensor", "FrcnnError", "Localizer", "MT19937", "Rect", "combine_and_flatten_parameters",
           "adam", "create_model", "create_objective", "duplo_cfg", "extract_roi_pooling_input", "imgnet_cfg", "manualSeed", "nag", "nms", "soft_nms", "box_vote", "proposal_targets", "roi_hard_select", "cnet_loss", "cnet_loss_settings", "box_head", "box_head_settings", "class_boxes", "scoring_boxes", "eval_match", "average_precision_from_matches",
           "optimizer", "rmsprop", "sgd", "roi_pooling_settings", "roi_sampling_settings", "roi_window", "roi_windows", "vgg_large", "vgg_small"]
