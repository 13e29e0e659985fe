"""Weight pruning for the pruning baselines (reference Classification/pruner/): the mask operations of
pruner/utils.py on the flat arena.  The one-shot drivers `omp` / `synflow` belong to main_imp.py, which this build does
not carry."""
from .utils import *  # noqa: F401,F403
from .utils import __all__  # noqa: F401
