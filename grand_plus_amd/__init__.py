"""grand_plus_amd -- MI355X-native GFPush propagation-matrix precompute (GRAND+ hot path).

Only what the path needs lives here: `csrc/` (HIP kernels + the C ABI of
include/grandplus.h), the ctypes binding (`_native`), the host-side mirror of the
reference's `propagation.Graph` (`api.Graph`), the caller-side recipe helpers (`recipes`),
the multi-GPU seed-sharding driver (`sharded`), the tie-aware parity comparator (`parity`)
and the synthetic workload generator (`synth`).  The training-step pieces (`augment`, `mlp`, `objective`, `optim`) need
torch and are imported on demand; `ClipAdam` and `clip_grad_norm` of `optim` and `valid`, `predict`, `local_logits`, `eval_head`,
`eval_reduce`, `eval_tail` and `ValidGraph` of `evaluate`, `mag_prop_rows`, `valid_mag`, `valid_mag_plan`, `valid_mag_pass` and `predict_mag` of `mag`, `StepState` and `TrainStep` of `step`, `MagTrainStep` and `mag_trained_parameters` of `mag_step`, `RowGrad`, `BitmapRowGrad` and `DeferredRows` of `optim_rows` and `fit`, `Sampler` and `BestTracker` of `fit` are reachable from here by name, and stay out of `__all__` so that `from grand_plus_amd import *` loads neither torch nor the native library.
"""
from .api import Graph, algorithmic_bytes          # noqa: F401
from .recipes import RECIPES, Recipe, make_coef    # noqa: F401

__all__ = ["Graph", "algorithmic_bytes", "RECIPES", "Recipe", "make_coef"]


def __getattr__(name):                              # these need torch: loaded when first asked for
    if name in ("ClipAdam", "clip_grad_norm"):
        from . import optim
        return getattr(optim, name)
    if name in ("valid", "predict", "local_logits", "eval_head", "eval_reduce", "eval_tail", "ValidGraph"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("mag_prop_rows", "valid_mag", "valid_mag_plan", "valid_mag_pass", "predict_mag"):
        from . import mag
        return getattr(mag, name)
    if name in ("StepState", "TrainStep"):
        from . import step
        return getattr(step, name)
    if name in ("MagTrainStep", "mag_trained_parameters"):
        from . import mag_step
        return getattr(mag_step, name)
    if name in ("RowGrad", "BitmapRowGrad", "DeferredRows"):
        from . import optim_rows
        return getattr(optim_rows, name)
    if name in ("fit", "Sampler", "BestTracker"):
        import importlib
        module = importlib.import_module(".fit", __name__)
        return module if name == "fit" else getattr(module, name)   # the module shares its function's name: it is callable as it
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
