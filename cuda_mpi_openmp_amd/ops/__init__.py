"""Operators backed by hand-written gfx950 HIP kernels (GPU tensors) and the
OpenMP C references (CPU tensors) of libmpx."""

from .classify import class_stats, classify_
from .classify import plan as classify_plan
from .edge import ConvLauncher, conv, conv_rows, roberts, roberts_rgb
from .filters import Filter, get_filter, list_filters
from .linalg import (cholesky_factor, cholesky_factor_, cholesky_factor_batched, cholesky_factor_batched_,
                     cholesky_solve, cholesky_solve_, cholesky_solve_batched, cholesky_solve_batched_, logdet_spd,
                     logdet_spd_batched, solve_spd_batched, lu_factor,
                     lu_factor_, lu_factor_batched, lu_factor_batched_, lu_solve, lu_solve_, lu_solve_batched, lu_solve_batched_, lu_unpack, lu_unpack_batched, slogdet, slogdet_batched, solve,
                     solve_batched, solve_spd)
from .multigrid import (jacobi_relax, mg_prolong_add_, mg_prolong_cubic, mg_residual, mg_restrict, mg_tail,
                        tail_sweeps)
from .multigrid3d import (jacobi3d_relax, mg3_cubic_walk, mg3_prolong_add_, mg3_prolong_cubic, mg3_residual, mg3_restrict,
                          mg3_tail, mg3_walk)
from .sort import argsort, sort, sort_, sort_pairs_
from .stencil import jacobi3d_sweep, jacobi3d_tile, jacobi_sweep
from .vector import vsub

__all__ = [
    "class_stats",
    "classify_",
    "classify_plan",
    "conv",
    "ConvLauncher",
    "conv_rows",
    "roberts",
    "roberts_rgb",
    "Filter",
    "get_filter",
    "list_filters",
    "jacobi_sweep",
    "jacobi3d_sweep",
    "jacobi3d_tile",
    "jacobi_relax",
    "mg_residual",
    "mg_restrict",
    "mg_prolong_add_",
    "mg_prolong_cubic",
    "jacobi3d_relax",
    "mg3_residual",
    "mg3_restrict",
    "mg3_prolong_add_",
    "mg3_prolong_cubic",
    "mg3_cubic_walk",
    "mg3_walk",
    "mg_tail",
    "mg3_tail",
    "tail_sweeps",
    "argsort",
    "sort",
    "sort_",
    "sort_pairs_",
    "lu_factor",
    "lu_factor_",
    "lu_solve",
    "lu_solve_",
    "lu_unpack",
    "slogdet",
    "solve",
    "lu_factor_batched",
    "lu_factor_batched_",
    "lu_solve_batched",
    "lu_solve_batched_",
    "lu_unpack_batched",
    "slogdet_batched",
    "solve_batched",
    "cholesky_factor",
    "cholesky_factor_",
    "cholesky_solve",
    "cholesky_solve_",
    "solve_spd",
    "logdet_spd",
    "cholesky_factor_batched",
    "cholesky_factor_batched_",
    "cholesky_solve_batched",
    "cholesky_solve_batched_",
    "solve_spd_batched",
    "logdet_spd_batched",
    "vsub",
]
