"""snnflow -- MI355X-native (gfx950) LIFFireNet + event-warping hot path.

Drop-in for the reference's ``models.model`` (LIFFireNet family), its spiking cells,
``loss.flow.EventWarping`` and ``utils.iwe``; all compute runs in the HIP C-ABI library
``libsnnflow.so`` (include/snnflow.h).  Importing fails loudly if the library is missing.
"""
from . import _lib  # noqa: F401  (loads libsnnflow.so or raises)
from ._lib import SnnflowError, check_device_errors
from .cells import ConvLayer, Leaky, SNNtorch_ConvLIF, SNNtorch_ConvLIFRecurrent
from .norm import MPBN, TEBN
from .convlif import ConvLIF, ConvLIFRecurrent
from . import checkpoint, encodings  # noqa: F401  (checkpoint interchange, on-device event encodings)
from . import loader  # noqa: F401  (on-device batch preparation)
from .loader import BatchPreparer
from . import sequence  # noqa: F401  (on-device sequence reading: resident recordings -> raw windows)
from .sequence import EventSequence, SequenceLoader, SequenceReader
from . import vis  # noqa: F401  (on-device frame renderers and percentiles)
from . import profile  # noqa: F401  (on-device membrane profiling)
from .profile import VoltageProfiler
from .loss import EventWarping
from . import contrast  # noqa: F401  (on-device contrast-maximisation landscape for global flows)
from .contrast import best_global_flow, flow_heatmap, loss_landscape
from .metrics import AAE, AAE_Filtered, AAE_Weighted, AE_ofMeans, AEE, NAAE, NEE
from .optim import ClipAdam
from .model import LIFFireFlowNet, LIFFireFlowNet_short, LIFFireNet, LIFFireNet_short
from .unet import (SpikingMultiResUNetRecurrent, SpikingRecEVFlowNet, SpikingRecurrentConvLayer,
                   SpikingResidualBlock, SpikingUpsampleConvLayer)

__all__ = ["LIFFireNet", "LIFFireNet_short", "LIFFireFlowNet", "LIFFireFlowNet_short", "SNNtorch_ConvLIF",
           "SNNtorch_ConvLIFRecurrent", "ConvLIF", "ConvLIFRecurrent", "ConvLayer", "Leaky", "EventWarping", "AEE",
           "NEE", "AAE", "NAAE", "AE_ofMeans", "AAE_Weighted", "AAE_Filtered", "SpikingRecEVFlowNet",
           "SpikingMultiResUNetRecurrent", "SpikingRecurrentConvLayer", "SpikingResidualBlock", "SpikingUpsampleConvLayer",
           "ClipAdam", "SnnflowError", "check_device_errors", "BatchPreparer", "VoltageProfiler",
           "EventSequence", "SequenceReader", "SequenceLoader",
           "loss_landscape", "flow_heatmap", "best_global_flow"]
