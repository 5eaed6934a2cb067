from .distill import ArcFlowDistiller, DistillConfig  # noqa: F401
from .reducer import GradReducer, host_or_device, init_distributed  # noqa: F401
from . import checkpoint  # noqa: F401
from .evaluate import Evaluator, masked_metrics_from_sums, masked_ssim_from_sums, metrics_from_sums, ssim_from_sums  # noqa: F401
