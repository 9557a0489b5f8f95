"""m3vit_amd: MI355X (gfx950) implementation of the M3ViT MoE-ViT forward/backward hot path.

The compute lives in libm3vit_hip.so (hand-written HIP, C ABI in include/m3vit_hip.h);
this package is the host-side mirror of the reference's `fmoe`-shaped layer API.
"""
__version__ = "0.1.0"


def install_fmoe_shim():
    """Register m3vit_amd.fmoe as the top-level package `fmoe` (and its submodules) so that an
    unmodified reference checkout (`from fmoe.layers import FMoE, _fmoe_general_global_forward`, ...)
    binds to the HIP implementation.  Refuses to shadow a real fastmoe install."""
    import importlib
    import sys
    if "fmoe" in sys.modules and not getattr(sys.modules["fmoe"], "__m3vit_shim__", False):
        raise RuntimeError("a different `fmoe` package is already imported")
    pkg = importlib.import_module("m3vit_amd.fmoe")
    pkg.__m3vit_shim__ = True
    sys.modules["fmoe"] = pkg
    for sub in ("layers", "linear", "functions", "gates", "gates.base_gate", "gates.naive_gate", "distributed"):
        sys.modules["fmoe." + sub] = importlib.import_module("m3vit_amd.fmoe." + sub)
    return pkg


_LOSS_NAMES = ("SoftMaxwithLoss", "BalancedCrossEntropyLoss", "DepthLoss", "NormalsLoss", "SingleTaskLoss", "MultiTaskLoss",
               "get_loss")
_METER_NAMES = ("PerformanceMeter", "SemsegMeter", "HumanPartsMeter", "DepthMeter", "NormalsMeter", "SaliencyMeter", "EdgeMeter",
                "AverageMeter", "get_single_task_meter", "calculate_multi_task_performance", "get_output")
_SHARING_NAMES = ("ShareabilityPredictor", "Aggregation", "AggregationStage", "SharingRegularizationLoss", "SharingStage",
                  "TokenFFNStage")


def __getattr__(name):
    """the criterion modules of m3vit_amd.losses, the task meters of m3vit_amd.meters and the token sharing stage of
    m3vit_amd.sharing, importable from the package (loaded on first use: they need torch)"""
    if name in _LOSS_NAMES:
        from . import losses
        return getattr(losses, name)
    if name in _METER_NAMES:
        from . import meters
        return getattr(meters, name)
    if name in _SHARING_NAMES:
        from . import sharing
        return getattr(sharing, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
