"""ctypes binding of ``libmpx.so`` — the single native library (HIP kernels for
gfx950, OpenMP CPU references, host statistics) shared with the lab CLIs.

Import order matters on ROCm: PyTorch ships its own ``libamdhip64.so.7``. Loading
torch first makes the dynamic loader resolve libmpx's ``libamdhip64.so.7``
dependency to torch's already-loaded runtime (same SONAME), so device pointers,
streams and contexts are shared between torch tensors and mpx kernels.

The library is built in-tree (``make lib`` or ``__graft_entry__.build()``). On a
GPU path a missing library is an error, never a silent fallback.
"""

from __future__ import annotations

import ctypes
import os
import subprocess
import threading
from pathlib import Path

import torch  # noqa: F401  (must be loaded before libmpx; see module docstring)

_PKG_DIR = Path(__file__).resolve().parent
REPO_ROOT = _PKG_DIR.parent
# MPX_LIB_PATH: load another build of libmpx (kernel A/B runs: tools/*_ab.py)
LIB_PATH = Path(os.environ["MPX_LIB_PATH"]) if os.environ.get("MPX_LIB_PATH") else _PKG_DIR / "_lib" / "libmpx.so"

_lib = None
_lock = threading.Lock()

c_int, c_i64, c_size, c_vp = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
c_char_p = ctypes.c_char_p
_dp = ctypes.POINTER(ctypes.c_double)
_fp = ctypes.POINTER(ctypes.c_float)
_ip = ctypes.POINTER(ctypes.c_int)

# name -> (restype, argtypes)
_SIGNATURES = {
    "mpx_last_error": (c_char_p, []),
    "mpx_version": (c_char_p, []),
    "mpx_device_count": (c_int, [_ip]),
    "mpx_device_report": (c_int, [c_int, ctypes.c_char_p, c_size]),
    "mpx_stream_sync": (c_int, [c_vp]),
    "mpx_vsub_f64": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "mpx_vsub_f32": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "mpx_roberts": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "mpx_conv": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _fp, _fp, c_vp]),
    "mpx_conv_direct": (
        c_int,
        [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _fp, _fp, c_vp],
    ),
    "mpx_conv_set_band_min": (ctypes.c_longlong, [ctypes.c_longlong]),
    "mpx_conv_set_band_mode": (c_int, [c_int]),
    # (w, rows, k, anchor, resident, remote_rows, *seg, *opt) -> 0 wave / 1 band4 / 2 band16v
    "mpx_conv_band_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, _ip, _ip]),
    "mpx_conv_peer": (
        c_int,
        [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _fp, _fp, c_vp],
    ),
    "mpx_ipc_handle_size": (c_int, []),
    "mpx_ipc_get_handle": (c_int, [c_vp, c_vp, ctypes.POINTER(c_i64)]),
    "mpx_ipc_open": (c_int, [c_vp, ctypes.POINTER(c_vp)]),
    "mpx_ipc_open_dev": (c_int, [c_int, c_vp, ctypes.POINTER(c_vp)]),
    "mpx_ipc_close": (c_int, [c_vp]),
    "mpx_memcpy_d2d": (c_int, [c_vp, c_vp, c_i64, c_vp]),
    "mpx_filter_lookup": (c_int, [c_char_p, _ip, _ip, _ip, _fp, _fp]),
    "mpx_filter_name": (c_char_p, [c_int]),
    "mpx_class_stats": (c_int, [c_vp, c_int, c_int, c_int, _ip, _ip, _dp, _dp]),
    "mpx_classify": (c_int, [c_vp, c_i64, c_int, _dp, _dp, c_int, c_int, c_int, c_vp]),
    "mpx_comm_load": (c_int, [ctypes.c_char_p]),
    "mpx_comm_version": (c_int, []),
    "mpx_comm_unique_id": (c_int, [c_vp, c_int]),
    "mpx_comm_init": (c_int, [ctypes.POINTER(c_vp), c_int, c_int, c_vp, c_int, c_int]),
    "mpx_comm_destroy": (c_int, [c_vp]),
    "mpx_comm_rank": (c_int, [c_vp]),
    "mpx_comm_size": (c_int, [c_vp]),
    "mpx_comm_p2p_start": (c_int, [c_vp, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_vp),
                                   ctypes.POINTER(c_i64), ctypes.POINTER(c_int), c_vp]),
    "mpx_comm_p2p_wait": (c_int, [c_vp, c_vp]),
    "mpx_comm_p2p": (c_int, [c_vp, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_vp),
                             ctypes.POINTER(c_i64), ctypes.POINTER(c_int), c_vp]),
    "mpx_comm_allreduce": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "mpx_comm_check": (c_int, [c_vp]),
    "mpx_comm_abort": (c_int, [c_vp]),
    "mpx_comm_stream": (c_vp, [c_vp]),
    "mpx_classify_ex": (c_int, [c_vp, c_i64, c_int, _dp, _dp, c_int, c_int, c_int, c_vp, c_vp]),
    "mpx_classify_plan": (c_int, [c_int, _dp, _dp, c_int, ctypes.POINTER(ctypes.c_float)]),
    "mpx_classify_i8_params": (c_int, [c_int, _dp, _dp, c_vp, c_vp, c_vp, c_vp]),
    "mpx_classify_f16_params": (c_int, [c_int, _dp, _dp, c_vp, c_vp, c_vp]),
    "mpx_jacobi_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "mpx_jacobi_sync_bytes": (c_int, []),
    "mpx_jacobi_peer_sweep": (c_int, [c_int, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "mpx_jacobi_f32": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    # Poisson sweeps: (u, b, un, ...) with the right-hand side b laid out like u
    "mpx_jacobi_rhs_f64": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "mpx_jacobi_rhs_f32": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "mpx_jacobi_peer_sweep_rhs": (c_int, [c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "mpx_cpu_jacobi_rhs_f64": (ctypes.c_double, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int]),
    # Chebyshev steps: (u, b or NULL, un in-out, ..., omega, ...)
    "mpx_jacobi_accel_f64": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp, c_vp]),
    "mpx_jacobi_accel_f32": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp, c_vp]),
    "mpx_jacobi_peer_sweep_accel": (c_int, [c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, ctypes.c_double, c_vp,
                                            c_vp, c_vp]),
    "mpx_cpu_jacobi_accel_f64": (ctypes.c_double, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double]),
    # damped sweeps (multigrid smoother): (u, b or NULL, un out, cols, pitch, r0, r1, omega, resid, stream)
    "mpx_jacobi_relax_f64": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp, c_vp]),
    "mpx_jacobi_relax_f32": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp, c_vp]),
    "mpx_cpu_jacobi_relax_f64": (ctypes.c_double, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double]),
    # multigrid: residual (u, b or NULL, r, rows, cols, pitch_u, pitch_b, pitch_r, resid, stream),
    # restrict (r, bc, hc, wc, pitch_r, pitch_bc, stream), prolong_add (e, u, hc, wc, pitch_e, pitch_u, stream)
    "mpx_mg_residual_f64": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "mpx_mg_residual_f32": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "mpx_mg_restrict_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    "mpx_mg_restrict_f32": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    "mpx_mg_prolong_add_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    "mpx_mg_prolong_add_f32": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    "mpx_cpu_mg_residual_f64": (ctypes.c_double, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int]),
    "mpx_cpu_mg_restrict_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int]),
    "mpx_cpu_mg_prolong_add_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int]),
    "mpx_mg_prolong_cubic_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    "mpx_mg_prolong_cubic_f32": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    "mpx_cpu_mg_prolong_cubic_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int]),
    # 3-D sweeps: (u, b or NULL, un, nx, ny, k0, k1, [omega,] resid, stream)
    "mpx_jacobi3d_f64": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "mpx_jacobi3d_f32": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "mpx_jacobi3d_accel_f64": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp, c_vp]),
    "mpx_jacobi3d_accel_f32": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp, c_vp]),
    "mpx_jacobi3d_tile": (c_int, [c_int, c_int, c_int, _ip]),
    "mpx_cpu_jacobi3d_f64": (ctypes.c_double, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int]),
    "mpx_cpu_jacobi3d_accel_f64": (ctypes.c_double, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double]),
    # 3-D multigrid: relax (u, b or NULL, un, d, ny, nx, pitch, plane, k0, k1, omega, resid, stream),
    # residual (u, b or NULL, r, d, ny, nx, pitch_u, plane_u, pitch_b, plane_b, pitch_r, plane_r, resid, stream),
    # restrict (r, bc, dc, hc, wc, pitch_r, plane_r, pitch_bc, plane_bc, stream),
    # prolong_add (e, u, dc, hc, wc, pitch_e, plane_e, pitch_u, plane_u, stream); plane strides are int64
    "mpx_jacobi3d_relax_f64": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_int,
                                       ctypes.c_double, c_vp, c_vp]),
    "mpx_jacobi3d_relax_f32": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_int,
                                       ctypes.c_double, c_vp, c_vp]),
    "mpx_mg3_residual_f64": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64, c_int, c_i64,
                                     c_vp, c_vp]),
    "mpx_mg3_residual_f32": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64, c_int, c_i64,
                                     c_vp, c_vp]),
    "mpx_mg3_restrict_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64, c_vp]),
    "mpx_mg3_restrict_f32": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64, c_vp]),
    "mpx_mg3_prolong_add_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64, c_vp]),
    "mpx_mg3_prolong_add_f32": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64, c_vp]),
    "mpx_mg3_prolong_cubic_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64, c_vp]),
    "mpx_mg3_prolong_cubic_f32": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64, c_vp]),
    "mpx_mg3_walk": (c_int, [_ip]),
    "mpx_mg3_cubic_walk": (c_int, [_ip]),
    # the coarse levels of a V-cycle in one kernel: (levels, n, nu1, nu2, coarse_sweeps, omega, stream)
    "mpx_mg_tail_f64": (c_int, [c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp]),
    "mpx_mg_tail_f32": (c_int, [c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp]),
    "mpx_mg3_tail_f64": (c_int, [c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp]),
    "mpx_mg3_tail_f32": (c_int, [c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp]),
    "mpx_cpu_jacobi3d_relax_f64": (ctypes.c_double, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_int,
                                                     ctypes.c_double]),
    "mpx_cpu_mg3_residual_f64": (ctypes.c_double, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64,
                                                   c_int, c_i64]),
    "mpx_cpu_mg3_restrict_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64]),
    "mpx_cpu_mg3_prolong_add_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64]),
    "mpx_cpu_mg3_prolong_cubic_f64": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_i64, c_int, c_i64]),
    "mpx_cpu_threads": (c_int, []),
    "mpx_cpu_vsub_f64": (None, [c_vp, c_vp, c_vp, c_i64]),
    "mpx_cpu_vsub_f32": (None, [c_vp, c_vp, c_vp, c_i64]),
    "mpx_cpu_roberts": (None, [c_vp, c_vp, c_int, c_int]),
    "mpx_cpu_roberts_rgb": (None, [c_vp, c_vp, c_int, c_int]),
    "mpx_roberts_rgb": (c_int, [c_vp, c_vp, c_int, c_int, c_vp]),
    "mpx_cpu_conv": (None, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _fp, _fp]),
    "mpx_cpu_classify": (None, [c_vp, c_i64, c_int, _dp, _dp]),
    "mpx_cpu_jacobi_f64": (ctypes.c_double, [c_vp, c_vp, c_int, c_int, c_int, c_int]),
    "mpx_sort": (c_int, [c_vp, c_i64, c_int, c_vp]),
    "mpx_sort_workspace_bytes": (c_i64, [c_i64, c_int]),
    "mpx_sort_ws": (c_int, [c_vp, c_i64, c_int, c_vp, c_i64, c_vp]),
    "mpx_sort_ws_status": (c_int, [c_vp, c_i64, c_int]),
    "mpx_sort_lane_order_ok": (c_int, [c_vp]),
    "mpx_cpu_sort": (None, [c_vp, c_i64, c_int]),
    "mpx_sort_pairs_workspace_bytes": (c_i64, [c_i64, c_int]),
    "mpx_sort_pairs_ws": (c_int, [c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_i64, c_vp]),
    "mpx_cpu_sort_pairs": (None, [c_vp, c_vp, c_i64, c_int, c_int]),
    # lab4 LU: factor (a, n, pitch, piv, info, ws, ws_bytes, stream),
    # solve (lu, n, pitch, piv, b, nrhs, pitch_b, ws, ws_bytes, stream), phase (..., info, j0, phase, ws, ...)
    "mpx_lu_workspace_bytes": (c_i64, [c_int]),
    "mpx_lu_panel_width": (c_int, []),
    "mpx_lu_factor_f64": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "mpx_lu_solve_f64": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp, c_int, c_i64, c_vp, c_i64, c_vp]),
    "mpx_lu_phase_f64": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp, c_int, c_int, c_vp, c_i64, c_vp]),
    "mpx_cpu_lu_factor_f64": (None, [c_vp, c_int, c_i64, c_vp, c_vp]),
    "mpx_cpu_lu_solve_f64": (None, [c_vp, c_int, c_i64, c_vp, c_vp, c_int, c_i64]),
    # batched LU: factor (a, batch, n, pitch, stride, piv, info, ws, ws_bytes, stream),
    # solve (lu, batch, n, pitch, stride, piv, b, nrhs, pitch_b, stride_b, stream)
    "mpx_lu_batched_workspace_bytes": (c_i64, [c_int, c_int]),
    "mpx_lu_factor_batched_f64": (c_int, [c_vp, c_int, c_int, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "mpx_lu_solve_batched_f64": (c_int, [c_vp, c_int, c_int, c_i64, c_i64, c_vp, c_vp, c_int, c_i64, c_i64, c_vp]),
    "mpx_cpu_lu_factor_batched_f64": (None, [c_vp, c_int, c_int, c_i64, c_i64, c_vp, c_vp]),
    "mpx_cpu_lu_solve_batched_f64": (None, [c_vp, c_int, c_int, c_i64, c_i64, c_vp, c_vp, c_int, c_i64, c_i64]),
    # lab4 Cholesky (chol.hip): lower storage, no pivots, no workspace
    "mpx_chol_factor_f64": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp]),
    "mpx_chol_solve_f64": (c_int, [c_vp, c_int, c_i64, c_vp, c_int, c_i64, c_vp]),
    "mpx_chol_phase_f64": (c_int, [c_vp, c_int, c_i64, c_vp, c_int, c_int, c_vp]),
    "mpx_cpu_chol_factor_f64": (None, [c_vp, c_int, c_i64, c_vp]),
    "mpx_cpu_chol_solve_f64": (None, [c_vp, c_int, c_i64, c_vp, c_int, c_i64]),
    # batched Cholesky (chol_batched.hip): factor (a, batch, n, pitch, stride, info, stream),
    # solve (l, batch, n, pitch, stride, b, nrhs, pitch_b, stride_b, stream)
    "mpx_chol_factor_batched_f64": (c_int, [c_vp, c_int, c_int, c_i64, c_i64, c_vp, c_vp]),
    "mpx_chol_solve_batched_f64": (c_int, [c_vp, c_int, c_int, c_i64, c_i64, c_vp, c_int, c_i64, c_i64, c_vp]),
    "mpx_cpu_chol_factor_batched_f64": (None, [c_vp, c_int, c_int, c_i64, c_i64, c_vp]),
    "mpx_cpu_chol_solve_batched_f64": (None, [c_vp, c_int, c_int, c_i64, c_i64, c_vp, c_int, c_i64, c_i64]),
    # lab4 QR (qr.hip): factor (a, m, n, pitch, tau, info, ws, ws_bytes, stream),
    # apply (qr, m, n, pitch, tau, b, nrhs, pitch_b, transpose, ws, ws_bytes, stream),
    # rsolve (qr, n, pitch, b, nrhs, pitch_b, stream), phase (a, m, n, pitch, tau, info, j0, phase, ws, ...)
    "mpx_qr_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "mpx_qr_factor_f64": (c_int, [c_vp, c_int, c_int, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "mpx_qr_apply_f64": (c_int, [c_vp, c_int, c_int, c_i64, c_vp, c_vp, c_int, c_i64, c_int, c_vp, c_i64, c_vp]),
    "mpx_qr_rsolve_f64": (c_int, [c_vp, c_int, c_i64, c_vp, c_int, c_i64, c_vp]),
    "mpx_qr_plan": (c_int, [c_int, c_int, c_vp]),
    "mpx_qr_phase_f64": (c_int, [c_vp, c_int, c_int, c_i64, c_vp, c_vp, c_int, c_int, c_vp, c_i64, c_vp]),
    "mpx_cpu_qr_factor_f64": (None, [c_vp, c_int, c_int, c_i64, c_vp, c_vp]),
    "mpx_cpu_qr_apply_f64": (None, [c_vp, c_int, c_int, c_i64, c_vp, c_vp, c_int, c_i64, c_int]),
    "mpx_cpu_qr_rsolve_f64": (None, [c_vp, c_int, c_i64, c_vp, c_int, c_i64]),
    "mpx_rows_checksum":(c_int, [c_vp, c_i64, c_int, c_i64, c_int, c_vp, c_vp]),
    "mpx_peer_probe_run": (c_int, [c_vp, c_vp]),
    "mpx_halo_fetch_run": (c_int, [c_vp, c_vp]),
    "mpx_conv_stream_peer_ok": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "mpx_conv_stream_peer_run": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _fp,
                                         _fp, c_vp, c_vp]),
    "mpx_sync_alloc": (c_int, [c_i64, ctypes.POINTER(c_vp), _ip]),
    "mpx_sync_free": (c_int, [c_vp]),
    "mpx_sync_write": (c_int, [c_vp, c_int, ctypes.c_uint]),
    "mpx_sync_read": (c_int, [c_vp, c_int, ctypes.POINTER(ctypes.c_uint)]),
    "mpx_sync_clear": (c_int, [c_vp, c_i64]),
}

MG_TAIL_MAX_LEVELS = 16


class MgLevel(ctypes.Structure):
    """mpx_mg_level (capi.h): one level of a fused 2-D multigrid tail."""
    _fields_ = [("u", c_vp), ("un", c_vp), ("b", c_vp), ("r", c_vp), ("h", c_int), ("w", c_int), ("pitch", c_int)]


class Mg3Level(ctypes.Structure):
    """mpx_mg3_level (capi.h): one level of a fused 3-D multigrid tail."""
    _fields_ = [("u", c_vp), ("un", c_vp), ("b", c_vp), ("r", c_vp), ("d", c_int), ("h", c_int), ("w", c_int),
                ("pitch", c_int), ("plane", c_i64)]


# tuning-only entry points (kernel variants, copy probes, the exhaustive
# fast-sqrt self-test): libmpx_tune.so, built from native/tune/ and loaded only
# by tools/kbench.py and its tests, never by the production paths
TUNE_PATH = _PKG_DIR / "_lib" / "libmpx_tune.so"
_TUNE_SIGNATURES = {
    "mpx_conv_variant": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _fp, _fp, c_vp]),
    "mpx_selftest_fast_sqrt": (c_int, [c_vp, c_int, c_vp]),
    "mpx_strip_copy_probe": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp]),
    # lab5 radix variants / scatter probe (native/tune/sort_variants.hip)
    "mpx_sort_variant": (c_int, [c_vp, c_i64, c_int, c_vp, c_i64, c_int, c_vp]),
    "mpx_sort_scatter_probe": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_vp]),
    "mpx_sort_pairs_variant": (c_int, [c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_i64, c_int, c_vp]),
    # lab1 / Jacobi tuning variants (native/tune/{vsub,jacobi}_variants.hip)
    "mpx_vsub_variant": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_int, c_vp]),
    "mpx_jacobi_variant": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp]),
    # (u, b, un, cols, pitch, r0, r1, resid, fp64, R, nt, stream)
    "mpx_jacobi_rhs_variant": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_int,
                                       c_vp]),
    # (u, b or NULL, un in-out, cols, pitch, r0, r1, omega, resid, fp64, R, stream)
    "mpx_jacobi_accel_variant": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_double, c_vp, c_int,
                                         c_int, c_vp]),
    # (fp64, u, b or NULL, un, nx, ny, k0, k1, accel, omega, resid, form, ty, kz, stream)
    "mpx_jacobi3d_variant": (c_int, [c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, ctypes.c_double,
                                     c_vp, c_int, c_int, c_int, c_vp]),
}
_tune = None


class MpxError(RuntimeError):
    """A libmpx entry point returned a non-zero status."""


def build(quiet: bool = True) -> None:
    """Build libmpx.so in-tree with the repository Makefile (gfx950 cross-compile)."""
    jobs = str(min(8, os.cpu_count() or 1))
    res = subprocess.run(
        ["make", "-C", str(REPO_ROOT), "-j", jobs, "lib"],
        capture_output=quiet,
        text=True,
    )
    if res.returncode != 0:
        raise MpxError(f"building libmpx failed:\n{res.stdout}\n{res.stderr}")


def lib(auto_build: bool = True) -> ctypes.CDLL:
    """Return the loaded library, building it first if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not LIB_PATH.exists():
            if not auto_build:
                raise MpxError(f"{LIB_PATH} not built; run `make lib`")
            build()
        handle = ctypes.CDLL(str(LIB_PATH), mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
        return _lib


def tune_lib() -> ctypes.CDLL:
    """The tuning library (after libmpx, whose error state and runtime it shares)."""
    global _tune
    lib()
    with _lock:
        if _tune is None:
            if not TUNE_PATH.exists():
                raise MpxError(f"{TUNE_PATH} not built; run `make tune`")
            handle = ctypes.CDLL(str(TUNE_PATH), mode=ctypes.RTLD_GLOBAL)
            for name, (res, args) in _TUNE_SIGNATURES.items():
                fn = getattr(handle, name)
                fn.restype = res
                fn.argtypes = args
            _tune = handle
    return _tune


def available() -> bool:
    try:
        lib()
        return True
    except (OSError, MpxError):
        return False


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().mpx_last_error()
        raise MpxError(msg.decode() if msg else f"libmpx error {rc}")


def ptr(t: "torch.Tensor") -> int:
    return t.data_ptr()


def stream_of(t: "torch.Tensor") -> int:
    """hipStream_t of the current torch stream on t's device (0 for CPU)."""
    if t.is_cuda:
        return torch.cuda.current_stream(t.device).cuda_stream
    return 0


def f32_array(values) -> ctypes.Array:
    vals = list(values)
    return (ctypes.c_float * max(1, len(vals)))(*vals)


def f64_array(values) -> ctypes.Array:
    vals = list(values)
    return (ctypes.c_double * max(1, len(vals)))(*vals)


def i32_array(values) -> ctypes.Array:
    vals = list(values)
    return (ctypes.c_int * max(1, len(vals)))(*vals)
