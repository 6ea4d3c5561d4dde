"""Mirror of the reference package of the same name (hot-path members only)."""
from .nn_laplace import NN_Laplace  # noqa: F401
from .nn_swag import NN_SWAG  # noqa: F401
