"""ctypes binding of the C ABI in include/mi355opt.h (libmi355opt.so).

This is harness plumbing for tests/ and bench.py: the product is the shared library (HIP kernels
behind a C ABI) and the C++ template layer in optimization_amd/include/.  There is no CPU fallback:
if the library is missing or no GPU is present the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355OPT_LIB") or os.path.join(_HERE, "libmi355opt.so")  # MI355OPT_LIB: experiment builds

MI_OK = 0
STATUS = {0: "MI_OK", 1: "MI_ERR_INVALID_ARGUMENT", 2: "MI_ERR_HIP", 3: "MI_ERR_OOM",
          4: "MI_ERR_NO_DEVICE", 5: "MI_ERR_COMM", 6: "MI_ERR_INTERNAL", 7: "MI_DECLINED"}
KERNELS = ["none", "cg_init", "cg_dot3", "cg_scalar_a", "cg_update", "cg_scalar_b", "cg_pupdate",
           "csr_spmm", "stiefel_spmm_gram", "stiefel_gram_reduce", "stiefel_finish_dots",
           "stiefel_retract", "bsr3_spmv_dots", "blas1", "lobpcg_gram", "lobpcg_update",
           "lobpcg_residual", "stiefel_hess_fused", "comm_allreduce", "comm_halo", "so3_grad",
           "so3_residual", "so3_jac", "so3_jact", "so3_edge_weight", "so3_inc_reweight", "pgo_model",
           "pgo_grad", "pgo_hvp", "pgo_retract"]
KID = {k: i for i, k in enumerate(KERNELS)}
STPCG_EXIT = ["RESIDUAL", "MAXIT", "KERNEL", "BOUNDARY", "USER"]

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)
c_size_p = C.POINTER(C.c_size_t)
vp = C.c_void_p

APPLY_FN = C.CFUNCTYPE(C.c_int, vp, vp, vp)
# mi_stpcg_observer: (user, k, s, r, v, p, alpha) -> nonzero stops the solve
OBSERVER_FN = C.CFUNCTYPE(C.c_int, vp, C.c_size_t, vp, vp, vp, vp, C.c_double)
# mi_lsqr_observer: (user, k, x, xnorm, rbar_norm, Arnorm, Anorm, Acond) -> nonzero stops the solve
LSQR_OBSERVER_FN = C.CFUNCTYPE(C.c_int, vp, C.c_size_t, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double)


class PanelBlocks(C.Structure):
    """mi_panel_blocks (include/mi355opt.h): a panel as 1..3 column blocks that need not be adjacent"""
    _fields_ = [("nblocks", C.c_int), ("block", C.c_void_p * 3), ("cols", C.c_int * 3)]

    @classmethod
    def of(cls, blocks):
        pb = cls()
        pb.nblocks = len(blocks)
        for i, (v, c) in enumerate(blocks):
            pb.block[i] = v.h
            pb.cols[i] = c
        pb._keep = [v for v, _ in blocks]
        return pb


class FusedArgs(C.Structure):
    _fields_ = [("partials", C.POINTER(C.c_double)), ("partial_stride", C.c_size_t), ("max_rows", C.c_int),
                ("required_rows", C.c_int), ("stream", vp)]


APPLY_FUSED_FN = C.CFUNCTYPE(C.c_int, vp, vp, vp, C.POINTER(FusedArgs), C.POINTER(C.c_int))


class MiError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS.get(status, status)}: {msg}")
        self.status = status


class StpcgParams(C.Structure):
    _fields_ = [("Delta", C.c_double), ("max_iterations", C.c_size_t), ("kappa_fgr", C.c_double),
                ("theta", C.c_double), ("epsilon", C.c_double), ("run_ahead", C.c_int),
                ("constraint_At", C.c_int), ("defer_result", C.c_int)]


class StpcgResult(C.Structure):
    _fields_ = [("update_step_M_norm", C.c_double), ("num_iterations", C.c_size_t),
                ("exit_reason", C.c_int), ("hvp_calls", C.c_size_t), ("rv_final", C.c_double),
                ("precon_status", C.c_int)]


class LsqrParams(C.Structure):
    _fields_ = [("max_iterations", C.c_size_t), ("lam", C.c_double), ("btol", C.c_double), ("Atol", C.c_double),
                ("Acond_limit", C.c_double), ("Delta", C.c_double), ("run_ahead", C.c_int)]


class LsqrResult(C.Structure):
    _fields_ = [("xnorm", C.c_double), ("num_iterations", C.c_size_t), ("exit_reason", C.c_int),
                ("rbar_norm", C.c_double), ("Arnorm", C.c_double), ("Anorm", C.c_double), ("Acond", C.c_double),
                ("operator_applications", C.c_size_t)]


LSQR_EXIT = ["MAXIT", "S1", "S2", "S3", "S4", "TRIVIAL"]


class PgoTransInfo(C.Structure):
    """mi_pgo_trans_info"""
    _fields_ = [("iterations", C.c_size_t), ("exit_reason", C.c_int), ("objective", C.c_double),
                ("relative_residual", C.c_double), ("max_residual", C.c_double)]


class StpcgTrace(C.Structure):
    _fields_ = [("cap", C.c_size_t), ("len", C.c_size_t), ("alpha", c_double_p), ("beta", c_double_p),
                ("kappa", c_double_p), ("rv", c_double_p)]


_lib = None


def load():
    """Load libmi355opt.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} not found: run `python -m optimization_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.mi_version.restype = C.c_char_p
    L.mi_last_error.restype = C.c_char_p
    L.mi_status_string.restype = C.c_char_p
    L.mi_status_string.argtypes = [C.c_int]
    L.mi_kernel_name.restype = C.c_char_p
    L.mi_kernel_name.argtypes = [C.c_int]
    sigs = {
        "mi_device_count": [C.POINTER(C.c_int)],
        "mi_ctx_create": [C.c_int, C.POINTER(vp)],
        "mi_ctx_destroy": [vp],
        "mi_ctx_sync": [vp],
        "mi_ctx_set_option": [vp, C.c_char_p, C.c_long],
        "mi_ctx_sync_count": [vp, c_size_p],
        "mi_ctx_fusion_counters": [vp, C.POINTER(FusionCounters)],
        "mi_ctx_fusion_counters_reset": [vp],
        "mi_ctx_note_generic": [vp, C.c_int, C.c_char_p],
        "mi_op_create_compose": [vp, vp, vp, C.POINTER(vp)],
        "mi_ctx_stream": [vp, C.POINTER(vp)],
        "mi_ctx_device_name": [vp, C.c_char_p, C.c_size_t],
        "mi_ctx_pool_bytes": [vp, c_size_p],
        "mi_ktime_enable": [vp, C.c_int, C.c_int],
        "mi_ktime_reset": [vp],
        "mi_ktime_read": [vp, C.c_int, c_size_p, c_double_p],
        "mi_range_push": [C.c_char_p],
        "mi_range_pop": [],
        "mi_timer_start": [vp],
        "mi_timer_stop": [vp, c_double_p],
        "mi_vec_create": [vp, C.c_size_t, C.POINTER(vp)],
        "mi_vec_destroy": [vp],
        "mi_vec_len": [vp, c_size_p],
        "mi_vec_data": [vp, C.POINTER(vp)],
        "mi_vec_touch": [vp],
        "mi_vec_upload": [vp, c_double_p, C.c_size_t],
        "mi_vec_download": [vp, c_double_p, C.c_size_t],
        "mi_vec_copy": [vp, vp],
        "mi_vec_fill": [vp, C.c_double],
        "mi_vec_scale": [vp, C.c_double],
        "mi_vec_div": [vp, C.c_double],
        "mi_vec_scale_to": [vp, C.c_double, vp],
        "mi_vec_axpy": [vp, C.c_double, vp],
        "mi_vec_axpby": [vp, C.c_double, vp, C.c_double, vp],
        "mi_vec_dot": [vp, vp, c_double_p],
        "mi_vec_dot_batch": [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), c_double_p],
        "mi_csr_create": [vp, C.c_size_t, C.c_size_t, c_int32_p, c_int32_p, c_double_p, C.POINTER(vp)],
        "mi_csr_destroy": [vp],
        "mi_csr_spmm": [vp, C.c_int, vp, vp],
        "mi_op_create_callback": [vp, C.c_size_t, APPLY_FN, vp, C.POINTER(vp)],
        "mi_op_create_callback_rect": [vp, C.c_size_t, C.c_size_t, APPLY_FN, vp, C.POINTER(vp)],
        "mi_op_create_callback_fused": [vp, C.c_size_t, APPLY_FN, APPLY_FUSED_FN, vp, C.POINTER(vp)],
        "mi_lsqr_default_params": [C.POINTER(LsqrParams)],
        "mi_lsqr": [vp, vp, vp, vp, C.POINTER(LsqrParams), vp, C.POINTER(LsqrResult)],
        "mi_op_create_diag": [vp, vp, C.POINTER(vp)],
        "mi_op_create_csr": [vp, vp, C.c_int, C.POINTER(vp)],
        "mi_op_apply": [vp, vp, vp],
        "mi_op_dims": [vp, c_size_p, c_size_p],
        "mi_op_destroy": [vp],
        "mi_precon_create_callback": [vp, C.c_size_t, APPLY_FN, vp, C.POINTER(vp)],
        "mi_precon_create_diag": [vp, vp, C.POINTER(vp)],
        "mi_precon_create_block3": [vp, vp, C.POINTER(vp)],
        "mi_precon_apply": [vp, vp, vp],
        "mi_precon_create_constraint": [vp, C.c_size_t, C.c_size_t, vp, vp, C.POINTER(vp)],
        "mi_precon_create_constraint_csr": [vp, C.c_size_t, C.c_size_t, c_int32_p, c_int32_p, c_double_p, vp, C.c_double,
                                            C.c_size_t, C.POINTER(vp)],
        "mi_precon_constraint_info": [vp, c_size_p, c_double_p, c_double_p, C.POINTER(C.c_int)],
        "mi_precon_constraint_solve": [vp, vp, vp, vp],
        "mi_precon_constraint_At": [vp, vp, vp],
        "mi_precon_destroy": [vp],
        "mi_stpcg": [vp, vp, vp, vp, C.POINTER(StpcgParams), vp, C.POINTER(StpcgResult),
                     C.POINTER(StpcgTrace)],
        "mi_stpcg_observed": [vp, vp, vp, vp, C.POINTER(StpcgParams), OBSERVER_FN, vp, vp, C.POINTER(StpcgResult),
                              C.POINTER(StpcgTrace)],
        "mi_stpcg_observer_available": [vp, C.POINTER(C.c_char_p)],
        "mi_lsqr_observed": [vp, vp, vp, vp, C.POINTER(LsqrParams), LSQR_OBSERVER_FN, vp, vp, C.POINTER(LsqrResult)],
        "mi_lsqr_observer_available": [vp, C.POINTER(C.c_char_p)],
        "mi_stiefel_gram": [vp, C.c_size_t, C.c_int, vp, vp, c_double_p],
        "mi_stiefel_project": [vp, C.c_size_t, C.c_int, vp, vp, vp],
        "mi_stiefel_retract": [vp, C.c_size_t, C.c_int, vp, vp, vp],
        "mi_stiefel_rq_create": [vp, vp, C.c_size_t, C.c_int, C.POINTER(vp)],
        "mi_stiefel_rq_destroy": [vp],
        "mi_stiefel_rq_objective": [vp, vp, c_double_p],
        "mi_stiefel_rq_model": [vp, vp, vp, C.POINTER(vp)],
        "mi_stiefel_rq_trial": [vp, vp, vp, vp, vp, c_double_p],
        "mi_stiefel_rq_armijo_trial": [vp, vp, vp, C.c_double, vp, vp, c_double_p],
        "mi_stiefel_rq_precon": [vp, vp, vp, C.POINTER(vp)],
        "mi_so3n_create": [vp, C.c_size_t, C.c_size_t, c_int32_p, c_int32_p, c_double_p, c_double_p,
                           C.POINTER(vp)],
        "mi_so3n_destroy": [vp],
        "mi_so3n_objective": [vp, vp, c_double_p],
        "mi_so3n_model": [vp, vp, vp, C.POINTER(vp), C.POINTER(vp)],
        "mi_so3n_retract": [vp, vp, vp, vp],
        "mi_so3n_trial": [vp, vp, vp, vp, C.c_int, vp, c_double_p],
        "mi_so3n_gradient": [vp, vp, vp],
        "mi_so3n_armijo_trial": [vp, vp, vp, C.c_double, vp, vp, c_double_p],
        "mi_so3n_residual": [vp, vp, vp, c_double_p],
        "mi_so3n_jacobian": [vp, vp, C.POINTER(vp), C.POINTER(vp)],
        "mi_so3n_gn_scaling": [vp, C.POINTER(vp)],
        "mi_so3n_certificate": [vp, vp, C.POINTER(vp), c_double_p],
        "mi_so3n_cert_apply": [vp, C.c_int, vp, vp],
        "mi_so3n_cert_apply_blocks": [vp, C.POINTER(PanelBlocks), vp],
        "mi_so3n_cert_null_panel": [vp, C.POINTER(vp)],
        "mi_so3n_laplacian": [vp, C.POINTER(vp)],
        "mi_so3n_lap_jacobi": [vp, C.c_int, vp, vp],
        "mi_so3n_round": [vp, vp, vp, c_double_p],
        "mi_so3n_project": [vp, vp, vp, c_double_p],
        "mi_so3n_reweight": [vp, vp, C.c_int, C.c_double, c_double_p],
        "mi_so3n_weights": [vp, c_double_p],
        "mi_pgo_trans_create": [vp, C.c_size_t, C.c_size_t, c_int32_p, c_int32_p, c_double_p, c_double_p, C.c_longlong,
                                C.POINTER(vp)],
        "mi_pgo_trans_destroy": [vp],
        "mi_pgo_trans_rhs": [vp, vp, vp],
        "mi_pgo_trans_operator": [vp, C.POINTER(vp), C.POINTER(vp)],
        "mi_pgo_trans_residual": [vp, vp, vp, vp, c_double_p],
        "mi_pgo_trans_solve": [vp, vp, C.c_double, C.c_size_t, vp, C.POINTER(PgoTransInfo)],
        "mi_pgo_create": [vp, C.c_size_t, C.c_size_t, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p,
                          C.POINTER(vp)],
        "mi_pgo_destroy": [vp],
        "mi_pgo_objective": [vp, vp, c_double_p],
        "mi_pgo_gradient": [vp, vp, vp],
        "mi_pgo_model": [vp, vp, vp, C.POINTER(vp), C.POINTER(vp)],
        "mi_pgo_retract": [vp, vp, vp, vp],
        "mi_pgo_trial": [vp, vp, vp, vp, C.c_int, vp, c_double_p],
        "mi_debug_pgo_pack": [C.c_size_t, C.c_size_t, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p,
                              c_size_p, C.POINTER(vp), c_size_p, c_size_p],
        "mi_debug_pgo_hvp_dots": [vp, vp, vp, c_double_p],
        "mi_debug_pgo_blocks": [vp, C.c_int, c_double_p, C.c_size_t, c_size_p, c_size_p],
        "mi_stpcg_collect": [vp, C.POINTER(StpcgResult)],
        "mi_lobpcg_gram": [vp, C.c_size_t, C.c_int, C.c_int, vp, vp, c_double_p],
        "mi_lobpcg_update": [vp, C.c_size_t, C.c_int, C.c_int, vp, c_double_p, C.c_int, vp],
        "mi_lobpcg_update2": [vp, C.c_size_t, C.c_int, C.c_int, vp, c_double_p, C.c_int, vp, C.c_int, vp],
        "mi_lobpcg_residual": [vp, C.c_size_t, C.c_int, vp, vp, vp, c_double_p, vp, c_double_p,
                               c_double_p],
        "mi_rayleigh_ritz": [C.c_int, c_double_p, c_double_p, c_double_p, c_double_p],
        "mi_rayleigh_ritz_lowest": [C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p],
        "mi_csr_spmm_colmajor": [vp, C.c_int, vp, vp],
        "mi_csr_spmm_colmajor_residual": [vp, C.c_int, vp, c_double_p, vp, vp, c_double_p, c_double_p],
        "mi_lobpcg_gram_split": [vp, C.c_size_t, C.c_int, vp, C.c_int, vp, vp, c_double_p],
        "mi_debug_window_runs": [C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)],
        "mi_lobpcg_gram_pair": [vp, C.c_size_t, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp, c_double_p, c_double_p],
        "mi_lobpcg_gram_pair_sym": [vp, C.c_size_t, C.c_int, vp, C.c_int, vp, vp, c_double_p, c_double_p],
        "mi_lobpcg_gram_pair_sym_blocks": [vp, C.c_size_t, vp, C.c_int, vp, vp, c_double_p, c_double_p],
        "mi_lobpcg_gram_pair_gen_blocks": [vp, C.c_size_t, vp, vp, vp, c_double_p, c_double_p],
        "mi_lobpcg_gram_pair_sym_tblocks": [vp, C.c_size_t, vp, vp, c_double_p, c_double_p],
        "mi_lobpcg_update2_blocks": [vp, C.c_size_t, vp, C.c_int, c_double_p, C.c_int, vp, C.c_int, vp],
        "mi_csr_spmm_colmajor_blocks": [vp, vp, vp],
        "mi_panel_rowscale": [vp, C.c_size_t, C.c_int, vp, vp, vp],
        "mi_vec_view": [vp, C.c_size_t, C.c_size_t, C.POINTER(vp)],
        "mi_comm_unique_id": [C.POINTER(C.c_ubyte)],
        "mi_comm_init": [vp, C.c_int, C.c_int, C.POINTER(C.c_ubyte)],
        "mi_comm_finalize": [vp],
        "mi_comm_info": [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "mi_comm_rccl_count": [vp, C.POINTER(C.c_int)],
        "mi_comm_ipc_export": [vp, C.POINTER(C.c_ubyte)],
        "mi_comm_ipc_attach": [vp, C.c_int, C.c_int, C.POINTER(C.c_ubyte)],
        "mi_comm_ipc_selftest": [vp, C.POINTER(C.c_int)],
        "mi_comm_ipc_enable": [vp, C.c_int],
        "mi_comm_ipc_error": [vp, C.POINTER(C.c_int)],
        "mi_comm_kernel_launches": [vp, C.POINTER(C.c_ulonglong)],
        "mi_comm_ipc_fold": [vp, C.c_int],
        "mi_debug_csr_window_info": [vp, c_size_p],
        "mi_debug_csr_format_info": [vp, c_size_p],
        "mi_debug_so3n_info": [vp, c_size_p],
        "mi_debug_op_apply_sub_scaled": [vp, vp, C.c_double, C.c_int, vp, c_double_p],
        "mi_debug_time_fused_apply": [vp, vp, vp, C.c_int, c_double_p],
        "mi_debug_set_rank": [vp, C.c_int, C.c_int],
        "mi_debug_csr_set_halo": [vp, C.c_int, c_double_p],
        "mi_csr_create_sharded": [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, c_int32_p,
                                  c_int64_p, c_double_p, c_size_p, C.POINTER(vp)],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = args
    L.mi_stpcg_default_params.restype = None
    L.mi_lsqr_default_params.restype = None
    L.mi_stpcg_default_params.argtypes = [C.POINTER(StpcgParams)]
    _lib = L
    return L


class FusionCounters(C.Structure):
    _fields_ = [(k, C.c_ulonglong) for k in ("fused_stpcg_solves", "generic_stpcg_solves", "fused_lsqr_solves",
                                             "generic_lsqr_solves", "fused_trial_steps", "generic_trial_steps",
                                             "generic_inner_products")]


def check(status):
    if status != MI_OK:
        raise MiError(status, load().mi_last_error().decode())


def window_runs(ntiles, max_wgs, num_cu=256, far_stride=0):
    """run plan of the LDS-window kernels (host-only, mi_debug_window_runs): array of run starts + the end"""
    L = load()
    cap = max(ntiles, max_wgs, 1) + 2
    buf = (C.c_int * cap)()
    nb = C.c_int(0)
    check(L.mi_debug_window_runs(ntiles, max_wgs, num_cu, far_stride, buf, cap, C.byref(nb)))
    return np.array(buf[:nb.value + 1], dtype=np.int64)


def stiefel_hess_form_fn():
    """mi_debug_stiefel_hess_form, bound on first use (an older experiment build loaded through MI355OPT_LIB lacks it)"""
    fn = load().mi_debug_stiefel_hess_form
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return fn


def stiefel_hess_form(p, gram_count, traits, switches):
    """launch plan of the Stiefel one-pass Hessian (host-only, mi_debug_stiefel_hess_form): the 14 numbers of `out`,
    or None where the library answers with an error"""
    out = (C.c_int * 14)()
    st = stiefel_hess_form_fn()(p, gram_count, (C.c_size_t * 9)(*traits), (C.c_int * 9)(*switches), out)
    return list(out) if st == MI_OK else None


def lobpcg_gram_plan_fn():
    """mi_debug_lobpcg_gram_plan(kind, in, out), bound on first use; the kinds and their numbers are in mi355opt.h"""
    fn = load().mi_debug_lobpcg_gram_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, c_size_p, c_size_p]
    return fn


def lobpcg_update_plan(m, cols, kc, Cmat, no_update_mfma=False):
    """plan of Y = S C and the packed coefficients (host-only, mi_debug_lobpcg_update_plan): (all_mfma, steps as rows
    of [block, first, four basis columns or -1], chunks as rows of [c0, width, offset], Ct).  Cmat: Fortran-ordered,
    at least sum(cols) rows (its leading dimension may be larger), kc columns."""
    fn = load().mi_debug_lobpcg_update_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, c_double_p, C.c_int, C.POINTER(C.c_int),
                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p,
                   C.c_size_t, c_size_p]
    assert Cmat.flags.f_contiguous and Cmat.dtype == np.float64 and Cmat.shape[1] >= kc
    cap = 96 * 96 * 2
    mf, ns, nc, n = C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    steps, chunks, Ct = (C.c_int * (18 * 6))(), (C.c_int * 12)(), np.full(cap, np.nan)
    check(fn(m, kc, len(cols), (C.c_int * len(cols))(*cols), int(no_update_mfma), Cmat.ctypes.data_as(c_double_p),
             Cmat.shape[0], C.byref(mf), C.byref(ns), steps, C.byref(nc), chunks, Ct.ctypes.data_as(c_double_p), cap,
             C.byref(n)))
    return (bool(mf.value), np.array(steps[:6 * ns.value], dtype=np.int64).reshape(-1, 6),
            np.array(chunks[:3 * nc.value], dtype=np.int64).reshape(-1, 3), Ct[:n.value].copy())


def lobpcg_sweep_plan(D, n, k, num_cu=256, sweep_zsegs=0):
    """grid of the plane-sweep panel product (host-only, mi_debug_lobpcg_sweep_plan): dict of the 7 numbers of `out`"""
    fn = load().mi_debug_lobpcg_sweep_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 7)()
    check(fn(D, n, k, num_cu, sweep_zsegs, out))
    return dict(zip(("ok", "tiles", "nst", "npass", "zsegs", "zs", "xgrid"), out))


def words16_option(text=None):
    """mi_debug_words16_option (host-only): Config::words16 of a context created with MI355OPT_WORDS16=text (None: unset)"""
    fn = load().mi_debug_words16_option
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    on = C.c_int(-1)
    check(fn(None if text is None else text.encode(), C.byref(on)))
    return bool(on.value)


def csr_shard_plan(n_global, world_size, rank, row_starts, col_global):
    """Host-only (no GPU): (col_local int32, need_lo, need_hi) for this rank's slab of a row-sharded matrix."""
    L = load()
    L.mi_csr_shard_plan.restype = C.c_int
    L.mi_csr_shard_plan.argtypes = [C.c_size_t, C.c_int, C.c_int, c_size_p, C.c_size_t, c_int64_p, c_int32_p,
                                    c_size_p, c_size_p]
    col_global = np.ascontiguousarray(col_global, dtype=np.int64)
    starts = (C.c_size_t * len(row_starts))(*[int(x) for x in row_starts])
    col_local = np.zeros(col_global.size, dtype=np.int32)
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    check(L.mi_csr_shard_plan(n_global, world_size, rank, starts, col_global.size,
                              col_global.ctypes.data_as(c_int64_p), col_local.ctypes.data_as(c_int32_p),
                              C.byref(lo), C.byref(hi)))
    return col_local, lo.value, hi.value


def device_count():
    n = C.c_int(0)
    check(load().mi_device_count(C.byref(n)))
    return n.value


def _dp(a):
    return a.ctypes.data_as(c_double_p)


class Context:
    def __init__(self, device=0):
        self.L = load()
        self.h = vp()
        check(self.L.mi_ctx_create(device, C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.mi_ctx_destroy(self.h)
            self.h = vp()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        check(self.L.mi_ctx_sync(self.h))

    def set_option(self, name, value):
        """mi_ctx_set_option: one of the library's MI355OPT_<NAME> switches on this live context"""
        check(self.L.mi_ctx_set_option(self.h, name.encode(), int(value)))
        return self

    def sync_count(self):
        n = C.c_size_t(0)
        check(self.L.mi_ctx_sync_count(self.h, C.byref(n)))
        return n.value

    def fusion_counters(self, reset=False):
        """mi_ctx_fusion_counters: which side of the fusion boundary the work of this context ran on"""
        fc = FusionCounters()
        check(self.L.mi_ctx_fusion_counters(self.h, C.byref(fc)))
        if reset:
            check(self.L.mi_ctx_fusion_counters_reset(self.h))
        return {k: int(getattr(fc, k)) for k, _ in FusionCounters._fields_}

    def device_name(self):
        buf = C.create_string_buffer(256)
        check(self.L.mi_ctx_device_name(self.h, buf, 256))
        return buf.value.decode()

    # vectors ------------------------------------------------------------------------------
    def vec(self, n):
        return Vec(self, n)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64).ravel()
        v = Vec(self, arr.size)
        check(self.L.mi_vec_upload(v.h, _dp(arr), arr.size))
        return v

    def dot_batch(self, xs, ys):
        k = len(xs)
        X = (vp * k)(*[x.h for x in xs])
        Y = (vp * k)(*[y.h for y in ys])
        out = np.zeros(k)
        check(self.L.mi_vec_dot_batch(self.h, k, X, Y, _dp(out)))
        return out

    # timing ---------------------------------------------------------------------------------
    def timer_start(self):
        check(self.L.mi_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_double(0)
        check(self.L.mi_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def range_push(self, name):
        check(self.L.mi_range_push(name.encode()))

    def range_pop(self):
        check(self.L.mi_range_pop())

    def ktime_enable(self, name, on=True):
        check(self.L.mi_ktime_enable(self.h, KID[name], int(on)))

    def ktime_reset(self):
        check(self.L.mi_ktime_reset(self.h))

    def ktime_read(self, name):
        n = C.c_size_t(0)
        ms = C.c_double(0)
        check(self.L.mi_ktime_read(self.h, KID[name], C.byref(n), C.byref(ms)))
        return n.value, ms.value

    # operators ------------------------------------------------------------------------------
    def csr(self, n, rowptr, col, val):
        return Csr(self, n, rowptr, col, val)

    def csr_sharded(self, n_global, row_begin, row_end, rowptr, col_global, val, row_starts):
        A = Csr.__new__(Csr)
        A.ctx, A.L = self, self.L
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col_global = np.ascontiguousarray(col_global, dtype=np.int64)
        val = np.ascontiguousarray(val, dtype=np.float64)
        starts = (C.c_size_t * len(row_starts))(*[int(x) for x in row_starts])
        A.n, A.nnz = row_end - row_begin, int(rowptr[-1])
        A.h = vp()
        check(self.L.mi_csr_create_sharded(self.h, n_global, row_begin, row_end, A.nnz,
                                           rowptr.ctypes.data_as(c_int32_p),
                                           col_global.ctypes.data_as(c_int64_p), _dp(val), starts,
                                           C.byref(A.h)))
        return A

    def op_diag(self, d):
        h = vp()
        check(self.L.mi_op_create_diag(self.h, d.h, C.byref(h)))
        return Op(self, h, keep=[d])

    def op_csr(self, A, p):
        h = vp()
        check(self.L.mi_op_create_csr(self.h, A.h, p, C.byref(h)))
        op = Op(self, h, keep=[A])
        op.n_in = A.n * p
        return op

    def op_callback(self, n, fn):
        """fn(in_vec: Vec, out_vec: Vec) enqueues out = Op(in)."""
        def cb(_u, pin, pout):
            try:
                fn(Vec(self, 0, handle=vp(pin)), Vec(self, 0, handle=vp(pout)))
                return 0
            except Exception:  # noqa
                import traceback
                traceback.print_exc()
                return 6
        cfn = APPLY_FN(cb)
        h = vp()
        check(self.L.mi_op_create_callback(self.h, n, cfn, None, C.byref(h)))
        return Op(self, h, keep=[cfn])

    def op_callback_rect(self, n_in, n_out, fn):
        """mi_op_create_callback_rect: fn(in_vec: Vec of n_in, out_vec: Vec of n_out) enqueues out = Op(in)."""
        def cb(_u, pin, pout):
            try:
                fn(Vec(self, 0, handle=vp(pin)), Vec(self, 0, handle=vp(pout)))
                return 0
            except Exception:  # noqa
                import traceback
                traceback.print_exc()
                return 6
        cfn = APPLY_FN(cb)
        h = vp()
        check(self.L.mi_op_create_callback_rect(self.h, n_in, n_out, cfn, None, C.byref(h)))
        op = Op(self, h, keep=[cfn])
        op.n_in = n_in
        return op

    def op_callback_fused(self, n, fn, fused):
        """mi_op_create_callback_fused.  fn(in_vec, out_vec) enqueues out = Op(in); fused(in_vec, out_vec, args) does the
        same AND leaves the three curvature partial rows (args: FusedArgs), returning the number of rows written.  (A
        real client does both in a HIP kernel of its own: examples/stpcg_user_stencil.hip; from Python this serves the
        contract tests.)"""
        def cb(_u, pin, pout):
            try:
                fn(Vec(self, 0, handle=vp(pin)), Vec(self, 0, handle=vp(pout)))
                return 0
            except Exception:  # noqa
                import traceback
                traceback.print_exc()
                return 6

        def cbf(_u, pin, pout, args, rows):
            try:
                rows[0] = int(fused(Vec(self, 0, handle=vp(pin)), Vec(self, 0, handle=vp(pout)), args.contents))
                return 0
            except Exception:  # noqa
                import traceback
                traceback.print_exc()
                return 6
        c1, c2 = APPLY_FN(cb), APPLY_FUSED_FN(cbf)
        h = vp()
        check(self.L.mi_op_create_callback_fused(self.h, n, c1, c2, None, C.byref(h)))
        return Op(self, h, keep=[c1, c2])

    def precon_diag(self, dinv):
        h = vp()
        check(self.L.mi_precon_create_diag(self.h, dinv.h, C.byref(h)))
        return Precon(self, h, keep=[dinv])

    def precon_block3(self, inv_blocks):
        h = vp()
        check(self.L.mi_precon_create_block3(self.h, inv_blocks.h, C.byref(h)))
        return Precon(self, h, keep=[inv_blocks])

    def precon_constraint(self, A, Minv):
        """mi_precon_create_constraint: A (m x n numpy, dense constraints), Minv (n, inverse of the diagonal M)"""
        A = np.ascontiguousarray(A, dtype=np.float64)
        m, n = A.shape
        Ad, Md = self.upload(A), self.upload(Minv)
        h = vp()
        check(self.L.mi_precon_create_constraint(self.h, n, m, Ad.h, Md.h, C.byref(h)))
        P = ConstraintPrecon(self, h, keep=[Ad, Md])
        P.m, P.n = m, n
        return P

    def precon_constraint_csr(self, A, Minv, inner_tol=0.0, inner_max_iterations=0):
        """mi_precon_create_constraint_csr: A scipy.sparse (m x n) or dense numpy (its non-zeros are taken)"""
        import scipy.sparse as sps
        A = sps.csr_matrix(A)
        A.sort_indices()
        m, n = A.shape
        Md = self.upload(Minv)
        rp = np.ascontiguousarray(A.indptr, dtype=np.int32)
        cl = np.ascontiguousarray(A.indices, dtype=np.int32)
        vl = np.ascontiguousarray(A.data, dtype=np.float64)
        h = vp()
        check(self.L.mi_precon_create_constraint_csr(self.h, n, m, rp.ctypes.data_as(c_int32_p),
                                                     cl.ctypes.data_as(c_int32_p), _dp(vl), Md.h, inner_tol,
                                                     inner_max_iterations, C.byref(h)))
        P = ConstraintPrecon(self, h, keep=[Md])
        P.m, P.n = m, n
        return P

    def precon_callback(self, n, fn):
        def cb(_u, pin, pout):
            try:
                fn(Vec(self, 0, handle=vp(pin)), Vec(self, 0, handle=vp(pout)))
                return 0
            except Exception:  # noqa
                import traceback
                traceback.print_exc()
                return 6
        cfn = APPLY_FN(cb)
        h = vp()
        check(self.L.mi_precon_create_callback(self.h, n, cfn, None, C.byref(h)))
        return Precon(self, h, keep=[cfn])

    # fused STPCG ------------------------------------------------------------------------------
    def stpcg(self, g, H, P=None, Delta=1.0, max_iterations=1000, kappa_fgr=.1, theta=.5,
              epsilon=1e-8, run_ahead=0, trace_cap=0, s_out=None, defer=False, constraint_At=False, observer=None):
        """defer=True: mi_stpcg returns without waiting for the device (s is valid in stream order); the scalar
        results come from stpcg_collect().
        observer: callable (k, s, r, v, p, alpha) -> bool, the reference's STPCGUserFunction (mi_stpcg_observed): called
        once per pass after alpha_k is known and before any update; s, r, v, p are non-owning Vec wrappers of the
        solve's own storage, valid for the duration of the call only (read them; v is r itself without a
        preconditioner); a true return stops the solve with s as it is (exit_reason 4).  An exception raised in it
        stops the solve and is re-raised here after the library call has returned."""
        prm = StpcgParams(Delta, max_iterations, kappa_fgr, theta, epsilon, run_ahead, int(constraint_At),
                          int(defer))
        res = StpcgResult()
        s = s_out if s_out is not None else Vec(self, g.n)
        tr = None
        arrs = {}
        if trace_cap:
            arrs = {k: np.zeros(trace_cap) for k in ("alpha", "beta", "kappa", "rv")}
            tr = StpcgTrace(trace_cap, 0, _dp(arrs["alpha"]), _dp(arrs["beta"]), _dp(arrs["kappa"]),
                            _dp(arrs["rv"]))
        if observer is not None:
            if defer:
                raise ValueError("an observed solve has no deferred result")
            raised = []

            def tramp(_user, k, sh, rh, vh, ph, alpha):
                try:
                    vs = [Vec(self, 0, handle=vp(h)) for h in (sh, rh, vh, ph)]
                    return 1 if observer(int(k), vs[0], vs[1], vs[2], vs[3], float(alpha)) else 0
                except BaseException as e:  # noqa: nothing may propagate through the C frames
                    raised.append(e)
                    return 1
            cfn = OBSERVER_FN(tramp)
            st = self.L.mi_stpcg_observed(self.h, g.h, H.h, P.h if P is not None else None, C.byref(prm), cfn, None,
                                          s.h, C.byref(res), C.byref(tr) if tr else None)
            if raised:
                raise raised[0]
            check(st)
        else:
            check(self.L.mi_stpcg(self.h, g.h, H.h, P.h if P is not None else None, C.byref(prm), s.h,
                                  C.byref(res), C.byref(tr) if tr else None))
        out = dict(s=s, M_norm=res.update_step_M_norm, iterations=res.num_iterations,
                   exit_reason=res.exit_reason, hvp_calls=res.hvp_calls, rv_final=res.rv_final,
                   precon_status=res.precon_status)
        if tr:
            out["trace"] = {k: v[:tr.len].copy() for k, v in arrs.items()}
        return out

    def stpcg_collect(self):
        res = StpcgResult()
        check(self.L.mi_stpcg_collect(self.h, C.byref(res)))
        return dict(M_norm=res.update_step_M_norm, iterations=res.num_iterations, exit_reason=res.exit_reason,
                    hvp_calls=res.hvp_calls, rv_final=res.rv_final, precon_status=res.precon_status)

    # fused LSQR ---------------------------------------------------------------------------------
    def lsqr_observer_available(self):
        """mi_lsqr_observer_available: (True, "") or (False, the reason the observed fused solve declines)"""
        why = C.c_char_p()
        st = self.L.mi_lsqr_observer_available(self.h, C.byref(why))
        return st == MI_OK, (why.value or b"").decode()

    def lsqr(self, A, At, b, x_out=None, observer=None, **kw):
        """mi_lsqr: A, At are Op handles (A: n_x -> n_y); kw: max_iterations, lam, btol, Atol, Acond_limit, Delta
        observer: callable (k, x, xnorm, rbar_norm, Arnorm, Anorm, Acond) -> bool, the reference's LSQRUserFunction
        (mi_lsqr_observed): called at the end of every pass that no stopping rule S1-S4 ended, with the loop index of
        the pass; x is a non-owning Vec wrapper of the solve's own storage, valid for the duration of the call only
        (read it); a true return stops the solve with x as it is (exit_reason 6, iterations = k).  An exception raised
        in it stops the solve and is re-raised here after the library call has returned."""
        prm = LsqrParams()
        self.L.mi_lsqr_default_params(C.byref(prm))
        for k, v in kw.items():
            if not hasattr(prm, k):
                raise AttributeError(k)
            setattr(prm, k, v)
        res = LsqrResult()
        x = x_out if x_out is not None else Vec(self, getattr(A, "n_in", None) or b.n)
        if observer is not None:
            raised = []

            def tramp(_user, k, xh, xnorm, rbar_norm, Arnorm, Anorm, Acond):
                try:
                    return 1 if observer(int(k), Vec(self, 0, handle=vp(xh)), float(xnorm), float(rbar_norm),
                                         float(Arnorm), float(Anorm), float(Acond)) else 0
                except BaseException as e:  # noqa: nothing may propagate through the C frames
                    raised.append(e)
                    return 1
            cfn = LSQR_OBSERVER_FN(tramp)
            st = self.L.mi_lsqr_observed(self.h, A.h, At.h, b.h, C.byref(prm), cfn, None, x.h, C.byref(res))
            if raised:
                raise raised[0]
            check(st)
        else:
            check(self.L.mi_lsqr(self.h, A.h, At.h, b.h, C.byref(prm), x.h, C.byref(res)))
        return dict(x=x, xnorm=res.xnorm, iterations=res.num_iterations, exit_reason=res.exit_reason,
                    rbar_norm=res.rbar_norm, Arnorm=res.Arnorm, Anorm=res.Anorm, Acond=res.Acond,
                    operator_applications=res.operator_applications)

    # Stiefel ----------------------------------------------------------------------------------
    def stiefel_gram(self, n, p, X, Z):
        G = np.zeros(p * p)
        check(self.L.mi_stiefel_gram(self.h, n, p, X.h, Z.h, _dp(G)))
        return G.reshape(p, p)

    def stiefel_project(self, n, p, X, Z):
        out = Vec(self, n * p)
        check(self.L.mi_stiefel_project(self.h, n, p, X.h, Z.h, out.h))
        return out

    def stiefel_retract(self, n, p, X, V):
        Y = Vec(self, n * p)
        check(self.L.mi_stiefel_retract(self.h, n, p, X.h, V.h, Y.h))
        return Y

    def stiefel_rq(self, A, n, p):
        return StiefelRQ(self, A, n, p)

    def so3n(self, N, ei, ej, Rt, w):
        return So3N(self, N, ei, ej, Rt, w)

    # LOBPCG panels (column-major m x k) ---------------------------------------------------------
    def lobpcg_gram(self, m, S, ka, T, kb):
        G = np.zeros((ka, kb), order="F")
        check(self.L.mi_lobpcg_gram(self.h, m, ka, kb, S.h, T.h, _dp(G)))
        return G

    def lobpcg_gram_split(self, m, S, k, T1, k1, T2):
        """S' [T1 | T2] with T in two panels (mi_lobpcg_gram_split)"""
        G = np.zeros((k, k), order="F")
        check(self.L.mi_lobpcg_gram_split(self.h, m, k, S.h, k1, T1.h, T2.h, _dp(G)))
        return G

    def lobpcg_gram_pair(self, m, S, k, Ta1, k1a, Ta2, Tb1, k1b, Tb2):
        """(S'[Ta1|Ta2], S'[Tb1|Tb2]) with one synchronisation; T?2 may be None (one panel of k columns)"""
        Ga, Gb = np.zeros((k, k), order="F"), np.zeros((k, k), order="F")
        check(self.L.mi_lobpcg_gram_pair(self.h, m, k, S.h, k1a, Ta1.h, Ta2.h if Ta2 is not None else None, k1b,
                                         Tb1.h, Tb2.h if Tb2 is not None else None, _dp(Ga), _dp(Gb)))
        return Ga, Gb

    def lobpcg_gram_pair_sym(self, m, S, k, Ta1, k1a, Ta2):
        """(S'[Ta1|Ta2] for a symmetric product, S'S) from one pass (mi_lobpcg_gram_pair_sym); Ta2 may be None"""
        Ga, Gb = np.zeros((k, k), order="F"), np.zeros((k, k), order="F")
        check(self.L.mi_lobpcg_gram_pair_sym(self.h, m, k, S.h, k1a, Ta1.h, Ta2.h if Ta2 is not None else None,
                                             _dp(Ga), _dp(Gb)))
        return Ga, Gb

    def lobpcg_gram_pair_sym_blocks(self, m, blocks, Ta1, k1a, Ta2):
        """the same on a basis held as column blocks [(panel or view, columns), ...] (mi_lobpcg_gram_pair_sym_blocks)"""
        k = sum(c for _, c in blocks)
        Ga, Gb = np.zeros((k, k), order="F"), np.zeros((k, k), order="F")
        pb = PanelBlocks.of(blocks)
        check(self.L.mi_lobpcg_gram_pair_sym_blocks(self.h, m, C.byref(pb), k1a, Ta1.h,
                                                    Ta2.h if Ta2 is not None else None, _dp(Ga), _dp(Gb)))
        return Ga, Gb

    def lobpcg_gram_pair_sym_tblocks(self, m, S_blocks, T_blocks):
        """(S'A(S), S'S), S and A(S) as column blocks (mi_lobpcg_gram_pair_sym_tblocks)"""
        k = sum(c for _, c in S_blocks)
        Ga, Gb = np.zeros((k, k), order="F"), np.zeros((k, k), order="F")
        ps, pt = PanelBlocks.of(S_blocks), PanelBlocks.of(T_blocks)
        check(self.L.mi_lobpcg_gram_pair_sym_tblocks(self.h, m, C.byref(ps), C.byref(pt), _dp(Ga), _dp(Gb)))
        return Ga, Gb

    def lobpcg_gram_pair_gen_blocks(self, m, S_blocks, AS_blocks, BS_blocks):
        """(S'A(S), S'B(S)) of the generalized problem, all three panels as column blocks (mi_lobpcg_gram_pair_gen_blocks)"""
        k = sum(c for _, c in S_blocks)
        Ga, Gb = np.zeros((k, k), order="F"), np.zeros((k, k), order="F")
        ps, pa, pb = PanelBlocks.of(S_blocks), PanelBlocks.of(AS_blocks), PanelBlocks.of(BS_blocks)
        check(self.L.mi_lobpcg_gram_pair_gen_blocks(self.h, m, C.byref(ps), C.byref(pa), C.byref(pb), _dp(Ga), _dp(Gb)))
        return Ga, Gb

    def lobpcg_update2_blocks(self, m, blocks, Cmat, k1):
        """mi_lobpcg_update2_blocks: S C for a basis held as column blocks, columns [0, k1) and the rest"""
        Cmat = np.asfortranarray(Cmat, dtype=np.float64)
        kc = Cmat.shape[1]
        Y1, Y2 = Vec(self, m * k1), Vec(self, m * max(kc - k1, 1))
        pb = PanelBlocks.of(blocks)
        check(self.L.mi_lobpcg_update2_blocks(self.h, m, C.byref(pb), kc, _dp(Cmat), Cmat.shape[0], Y1.h, k1,
                                              Y2.h if k1 < kc else None))
        return Y1, Y2

    def lobpcg_update(self, m, S, ks, Cmat):
        Cmat = np.asfortranarray(Cmat, dtype=np.float64)
        kc = Cmat.shape[1]
        Y = Vec(self, m * kc)
        check(self.L.mi_lobpcg_update(self.h, m, ks, kc, S.h, _dp(Cmat), Cmat.shape[0], Y.h))
        return Y

    def lobpcg_update2(self, m, S, ks, Cmat, k1):
        """columns [0, k1) of S C into one panel, the rest into another (mi_lobpcg_update2)"""
        Cmat = np.asfortranarray(Cmat, dtype=np.float64)
        kc = Cmat.shape[1]
        Y1, Y2 = Vec(self, m * k1), Vec(self, m * max(kc - k1, 1))
        check(self.L.mi_lobpcg_update2(self.h, m, ks, kc, S.h, _dp(Cmat), Cmat.shape[0], Y1.h, k1,
                                       Y2.h if k1 < kc else None))
        return Y1, Y2

    def lobpcg_residual(self, m, nx, AX, BX, X, theta):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        R = Vec(self, m * nx)
        rn, xn = np.zeros(nx), np.zeros(nx)
        check(self.L.mi_lobpcg_residual(self.h, m, nx, AX.h, BX.h, X.h, _dp(theta), R.h, _dp(rn), _dp(xn)))
        return R, rn, xn

    def rayleigh_ritz(self, A, B):
        A = np.asfortranarray(A, dtype=np.float64)
        B = np.asfortranarray(B, dtype=np.float64)
        n = A.shape[0]
        th = np.zeros(n)
        Cm = np.zeros((n, n), order="F")
        check(self.L.mi_rayleigh_ritz(n, _dp(A), _dp(B), _dp(th), _dp(Cm)))
        return th, Cm

    def rayleigh_ritz_lowest(self, A, B, k):
        A = np.asfortranarray(A, dtype=np.float64)
        B = np.asfortranarray(B, dtype=np.float64)
        n = A.shape[0]
        th = np.zeros(k)
        Cm = np.zeros((n, k), order="F")
        check(self.L.mi_rayleigh_ritz_lowest(n, k, _dp(A), _dp(B), _dp(th), _dp(Cm)))
        return th, Cm

    def panel_rowscale(self, m, k, d, X):
        Y = Vec(self, m * k)
        check(self.L.mi_panel_rowscale(self.h, m, k, d.h, X.h, Y.h))
        return Y

    # comm -------------------------------------------------------------------------------------
    def comm_unique_id(self):
        buf = (C.c_ubyte * 128)()
        check(self.L.mi_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, world_size, rank, uid):
        buf = (C.c_ubyte * 128)(*uid)
        check(self.L.mi_comm_init(self.h, world_size, rank, buf))

    # peer-memory exchange layer (include/mi355opt.h: mi_comm_ipc_*) -----------------------------
    IPC_HANDLE_BYTES = 64

    def comm_ipc_export(self):
        buf = (C.c_ubyte * self.IPC_HANDLE_BYTES)()
        check(self.L.mi_comm_ipc_export(self.h, buf))
        return bytes(buf)

    def comm_ipc_attach(self, world_size, rank, handles):
        assert len(handles) == world_size * self.IPC_HANDLE_BYTES
        buf = (C.c_ubyte * len(handles)).from_buffer_copy(handles)
        check(self.L.mi_comm_ipc_attach(self.h, world_size, rank, buf))

    def comm_ipc_selftest(self):
        ok = C.c_int(0)
        check(self.L.mi_comm_ipc_selftest(self.h, C.byref(ok)))
        return bool(ok.value)

    def comm_ipc_enable(self, on=True):
        check(self.L.mi_comm_ipc_enable(self.h, int(on)))

    def comm_ipc_error(self):
        e = C.c_int(0)
        check(self.L.mi_comm_ipc_error(self.h, C.byref(e)))
        return e.value

    def comm_ipc_fold(self, on):
        check(self.L.mi_comm_ipc_fold(self.h, int(on)))

    def comm_kernel_launches(self):
        """(scalar-exchange kernels, halo-push kernels, halo pushes folded into the producer kernel, of those: in the
        early form) so far"""
        out = (C.c_ulonglong * 4)()
        check(self.L.mi_comm_kernel_launches(self.h, out))
        return tuple(int(v) for v in out)

    def enable_peer_memory(self, world_size, rank, dist, force=False):
        """Collective bring-up of the peer-memory layer over a torch.distributed (gloo) control plane: export,
        gather handles, map, self-test; enabled only if EVERY rank succeeded at every step, else it stays off
        (RCCL then does the small exchanges).  Returns True when enabled.
        DEFAULT since r03: the layer is brought up and used whenever its collective self-test passes on every rank
        (bench.py additionally verifies the sharded data path through it and falls back to RCCL on any failure);
        MI355OPT_COMM=rccl keeps RCCL in charge.  force=True: the one-GPU multi-process tests, where RCCL cannot run."""
        import os

        def all_ok(flag, payload=None):
            lst = [None] * world_size
            dist.all_gather_object(lst, (bool(flag), payload))
            return all(f for f, _ in lst), [pl for _, pl in lst]

        if not force and os.environ.get("MI355OPT_COMM", "peer") == "rccl":
            return False
        try:
            handle, ok = self.comm_ipc_export(), True
        except MiError:
            handle, ok = b"\0" * self.IPC_HANDLE_BYTES, False
        ok, handles = all_ok(ok, handle)
        if not ok:
            return False
        try:
            self.comm_ipc_attach(world_size, rank, b"".join(handles))
            ok = True
        except MiError:
            ok = False
        ok, _ = all_ok(ok)
        if not ok:
            return False
        try:
            ok = self.comm_ipc_selftest()
        except MiError:
            ok = False
        ok, _ = all_ok(ok)
        self.comm_ipc_enable(ok)
        return ok

    def debug_set_rank(self, world_size, rank):
        """verification hook: act as `rank` of `world_size` without a communicator (tests only)"""
        check(self.L.mi_debug_set_rank(self.h, world_size, rank))

    def comm_finalize(self):
        check(self.L.mi_comm_finalize(self.h))

    def comm_rccl_count(self):
        """ranks of the RCCL communicator as RCCL reports them (ncclCommCount); 0 without one"""
        n = C.c_int(0)
        check(self.L.mi_comm_rccl_count(self.h, C.byref(n)))
        return n.value


class Vec:
    def __init__(self, ctx, n, handle=None):
        self.ctx = ctx
        self.L = ctx.L
        self.owned = handle is None
        if handle is None:
            self.h = vp()
            check(self.L.mi_vec_create(ctx.h, n, C.byref(self.h)))
            self.n = n
        else:
            self.h = handle
            m = C.c_size_t(0)
            check(self.L.mi_vec_len(self.h, C.byref(m)))
            self.n = m.value

    def __del__(self):
        try:
            if self.owned and self.h and self.ctx.h:
                self.L.mi_vec_destroy(self.h)
        except Exception:  # noqa
            pass

    def numpy(self):
        out = np.zeros(self.n)
        check(self.L.mi_vec_download(self.h, _dp(out), self.n))
        return out

    def set(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64).ravel()
        check(self.L.mi_vec_upload(self.h, _dp(arr), arr.size))
        return self

    def copy(self):
        v = Vec(self.ctx, self.n)
        check(self.L.mi_vec_copy(v.h, self.h))
        return v

    def fill(self, a):
        check(self.L.mi_vec_fill(self.h, a))
        return self

    def view(self, offset, n):
        """non-owning window [offset, offset + n) (mi_vec_view); this vector must outlive it"""
        h = vp()
        check(self.L.mi_vec_view(self.h, offset, n, C.byref(h)))
        v = Vec(self.ctx, 0, handle=h)
        v.owned, v.base = True, self      # the VIEW object is ours to destroy (not the storage)
        return v

    def data_ptr(self):
        p = vp()
        check(self.L.mi_vec_data(self.h, C.byref(p)))
        return p.value

    def touch(self):
        """announce a write made through data_ptr() outside the library (mi_vec_touch)"""
        check(self.L.mi_vec_touch(self.h))
        return self

    def scale(self, a):
        check(self.L.mi_vec_scale(self.h, a))
        return self

    def div(self, a):
        check(self.L.mi_vec_div(self.h, a))
        return self

    def scaled(self, a):
        z = Vec(self.ctx, self.n)
        check(self.L.mi_vec_scale_to(z.h, a, self.h))
        return z

    def axpy(self, a, x):
        check(self.L.mi_vec_axpy(self.h, a, x.h))
        return self

    def axpby(self, a, x, b, y):
        check(self.L.mi_vec_axpby(self.h, a, x.h, b, y.h))
        return self

    def dot(self, other):
        out = C.c_double(0)
        check(self.L.mi_vec_dot(self.h, other.h, C.byref(out)))
        return out.value


class Csr:
    def __init__(self, ctx, n, rowptr, col, val):
        self.ctx, self.L = ctx, ctx.L
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        self.n, self.nnz = n, int(rowptr[-1])
        self.h = vp()
        check(self.L.mi_csr_create(ctx.h, n, self.nnz, rowptr.ctypes.data_as(c_int32_p),
                                   col.ctypes.data_as(c_int32_p), _dp(val), C.byref(self.h)))

    def spmm(self, p, V, W=None):
        W = W if W is not None else Vec(self.ctx, self.n * p)
        check(self.L.mi_csr_spmm(self.h, p, V.h, W.h))
        return W

    def window_info(self):
        """(window half-width in chunks, widest slice, far stride D if the far columns are computed else 0, halo rows)"""
        out = (C.c_size_t * 4)()
        check(self.L.mi_debug_csr_window_info(self.h, out))
        return tuple(int(v) for v in out)

    def format_info(self):
        """mi_debug_csr_format_info: dict(packed, ntable, zidx (None: no 0.0 in the table), wk16, far_stride)"""
        out = (C.c_size_t * 5)()
        check(self.L.mi_debug_csr_format_info(self.h, out))
        zidx = None if out[2] == C.c_size_t(-1).value else int(out[2])
        return dict(packed=bool(out[0]), ntable=int(out[1]), zidx=zidx, wk16=bool(out[3]), far_stride=int(out[4]))

    def stiefel_hess_form(self, p, gram_count=-1):
        """mi_debug_stiefel_hess_form_of: the 14 numbers of the one-pass Hessian's launch plan for this matrix on its
        context as both stand (index 6, FAR: 2 = the 16-bit window words), or None where the library answers with an
        error"""
        fn = self.L.mi_debug_stiefel_hess_form_of
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_int)]
        out = (C.c_int * 14)()
        return list(out) if fn(self.ctx.h, self.h, p, gram_count, out) == MI_OK else None

    def debug_set_halo(self, p, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        check(self.L.mi_debug_csr_set_halo(self.h, p, _dp(rows)))

    def spmm_colmajor(self, k, X, Y=None):
        Y = Y if Y is not None else Vec(self.ctx, self.n * k)
        check(self.L.mi_csr_spmm_colmajor(self.h, k, X.h, Y.h))
        return Y

    def spmm_colmajor_blocks(self, blocks):
        """mi_csr_spmm_colmajor_blocks: A [block 0 | block 1 | ...] for column blocks [(panel or view, columns), ...]"""
        k = sum(c for _, c in blocks)
        Y = Vec(self.ctx, self.n * k)
        pb = PanelBlocks.of(blocks)
        check(self.L.mi_csr_spmm_colmajor_blocks(self.h, C.byref(pb), Y.h))
        return Y

    def spmm_colmajor_residual(self, nx, X, theta):
        """mi_csr_spmm_colmajor_residual: (AX, R, rnorm, xnorm)"""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        AX, R = Vec(self.ctx, self.n * nx), Vec(self.ctx, self.n * nx)
        rn, xn = np.zeros(nx), np.zeros(nx)
        check(self.L.mi_csr_spmm_colmajor_residual(self.h, nx, X.h, _dp(theta), AX.h, R.h, _dp(rn), _dp(xn)))
        return AX, R, rn, xn

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.L.mi_csr_destroy(self.h)
        except Exception:  # noqa
            pass


class Op:
    def __init__(self, ctx, h, keep=(), borrowed=False):
        self.ctx, self.L, self.h, self.keep, self.borrowed = ctx, ctx.L, h, list(keep), borrowed

    def apply(self, x, out=None):
        out = out if out is not None else Vec(self.ctx, getattr(self, "n_out", None) or x.n)
        check(self.L.mi_op_apply(self.h, x.h, out.h))
        return out

    def apply_sub_scaled(self, x, scale, inout, mode=0):
        """mi_debug_op_apply_sub_scaled: inout = Op(x) - scale inout in the operator's fused LSQR form; returns |inout|^2
        from the same pass (None when mode != 0: nothing must happen)"""
        s = C.c_double(float("nan"))
        check(self.L.mi_debug_op_apply_sub_scaled(self.h, x.h, float(scale), int(mode), inout.h, C.byref(s)))
        return s.value if mode == 0 else None

    def time_fused_apply(self, x, out, reps=200):
        """average us per application in the fused form mi_stpcg uses (mi_debug_time_fused_apply)"""
        us = C.c_double(0)
        check(self.L.mi_debug_time_fused_apply(self.h, x.h, out.h, reps, C.byref(us)))
        return us.value

    def __del__(self):
        try:
            if not self.borrowed and self.h and self.ctx.h:
                self.L.mi_op_destroy(self.h)
        except Exception:  # noqa
            pass


class Precon:
    def __init__(self, ctx, h, keep=()):
        self.ctx, self.L, self.h, self.keep = ctx, ctx.L, h, list(keep)

    def apply(self, r, out=None):
        out = out if out is not None else Vec(self.ctx, r.n)
        check(self.L.mi_precon_apply(self.h, r.h, out.h))
        return out

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.L.mi_precon_destroy(self.h)
        except Exception:  # noqa
            pass


class ConstraintPrecon(Precon):
    """The constraint preconditioner of the projected STPCG (mi_precon_create_constraint)."""

    def solve(self, r):
        """(v, lambda) = P(r)"""
        v, lam = Vec(self.ctx, self.n), Vec(self.ctx, self.m)
        check(self.L.mi_precon_constraint_solve(self.h, r.h, v.h, lam.h))
        return v, lam

    def At(self, lam):
        out = Vec(self.ctx, self.n)
        check(self.L.mi_precon_constraint_At(self.h, lam.h, out.h))
        return out

    def info(self):
        """(inner iterations of the last application, its relative residual, the worst one so far, status code: 0 ok,
        1 the inner iteration broke down, 2 it stopped at its iteration limit short of its tolerance): sparse form only.
        Never raises on a valid handle -- the code is an output."""
        it, last, worst, code = C.c_size_t(0), C.c_double(0), C.c_double(0), C.c_int(0)
        check(self.L.mi_precon_constraint_info(self.h, C.byref(it), C.byref(last), C.byref(worst), C.byref(code)))
        return it.value, last.value, worst.value, code.value


class _BorrowedPrecon(Precon):
    """A preconditioner owned by a problem object (never destroyed from Python)."""

    def __del__(self):
        pass


class So3N:
    """Chordal rotation averaging on SO(3)^N (mi_so3n_*)."""

    def __init__(self, ctx, N, ei, ej, Rt, w):
        self.ctx, self.L, self.N = ctx, ctx.L, N
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        ej = np.ascontiguousarray(ej, dtype=np.int32)
        Rt = np.ascontiguousarray(Rt, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        self.E = ei.size
        self.h = vp()
        check(self.L.mi_so3n_create(ctx.h, N, ei.size, ei.ctypes.data_as(c_int32_p),
                                    ej.ctypes.data_as(c_int32_p), _dp(Rt), _dp(w), C.byref(self.h)))

    def objective(self, R):
        f = C.c_double(0)
        check(self.L.mi_so3n_objective(self.h, R.h, C.byref(f)))
        return f.value

    def model(self, R, with_precon=True):
        """returns (grad Vec, Hessian Op, block-Jacobi Precon or None), all bound to R"""
        g = Vec(self.ctx, 3 * self.N)
        hop, pc = vp(), vp()
        check(self.L.mi_so3n_model(self.h, R.h, g.h, C.byref(hop), C.byref(pc) if with_precon else None))
        P = None
        if with_precon:
            P = Precon.__new__(Precon)
            P.ctx, P.L, P.h, P.keep = self.ctx, self.L, pc, [self, R]
            P.__class__ = _BorrowedPrecon
        return g, Op(self.ctx, hop, keep=[self, R], borrowed=True), P

    def retract(self, R, xi):
        Y = Vec(self.ctx, 9 * self.N)
        check(self.L.mi_so3n_retract(self.h, R.h, xi.h, Y.h))
        return Y

    def info(self):
        """mi_debug_so3n_info: dict(sinc_quat, gather_quat, nslices, nnzb, padded, model_grid)"""
        out = (C.c_size_t * 6)()
        check(self.L.mi_debug_so3n_info(self.h, out))
        return dict(sinc_quat=bool(out[0]), gather_quat=bool(out[1]), nslices=int(out[2]), nnzb=int(out[3]),
                    padded=int(out[4]), model_grid=int(out[5]))

    def trial(self, R, h, g, with_precon=True):
        """mi_so3n_trial: (R_trial Vec, dict(f, hh, gh, hHh, grad_sqnorm, precon_grad_sqnorm))"""
        Rt = Vec(self.ctx, 9 * self.N)
        out = np.zeros(6)
        check(self.L.mi_so3n_trial(self.h, R.h, h.h, g.h, int(with_precon), Rt.h, _dp(out)))
        return Rt, dict(f=out[0], hh=out[1], gh=out[2], hHh=out[3], grad_sqnorm=out[4], precon_grad_sqnorm=out[5])

    def gradient(self, R, out=None):
        """mi_so3n_gradient: grad f(R) (3N) through the gradient-only pass, or the copy of a trial's"""
        g = out if out is not None else Vec(self.ctx, 3 * self.N)
        check(self.L.mi_so3n_gradient(self.h, R.h, g.h))
        return g

    def residual(self, R, out=None, sqnorm=False):
        """mi_so3n_residual: F(R) (9E, sqrt(w_e) (R_j - R_i Rt_e) per edge); with sqnorm also |F|^2 of the same pass"""
        F = out if out is not None else Vec(self.ctx, 9 * self.E)
        s = C.c_double(0)
        check(self.L.mi_so3n_residual(self.h, R.h, F.h, C.byref(s) if sqnorm else None))
        return (F, s.value) if sqnorm else F

    def jacobian(self, R):
        """mi_so3n_jacobian: (dF Op 3N -> 9E, dF* Op 9E -> 3N), problem-owned, rebound by every call"""
        a, at = vp(), vp()
        check(self.L.mi_so3n_jacobian(self.h, R.h, C.byref(a), C.byref(at)))
        dF, dFt = Op(self.ctx, a, keep=[self], borrowed=True), Op(self.ctx, at, keep=[self], borrowed=True)
        dF.n_in, dF.n_out, dFt.n_in, dFt.n_out = 3 * self.N, 9 * self.E, 9 * self.E, 3 * self.N
        return dF, dFt

    def gn_scaling(self):
        """mi_so3n_gn_scaling: the diagonal operator diag(1 / sqrt(2 degw_i)) (3N), problem-owned"""
        m = vp()
        check(self.L.mi_so3n_gn_scaling(self.h, C.byref(m)))
        M = Op(self.ctx, m, keep=[self], borrowed=True)
        M.n_in = M.n_out = 3 * self.N
        return M

    def certificate(self, R):
        """mi_so3n_certificate: (So3NCertificate bound to a copy of what depends on R, dict(f, stationarity, trace_C));
        problem-owned, rebound by the next call"""
        h = vp()
        out = np.zeros(3)
        check(self.L.mi_so3n_certificate(self.h, R.h, C.byref(h), _dp(out)))
        return So3NCertificate(self, h), dict(f=out[0], stationarity=out[1], trace_C=out[2])

    def laplacian(self):
        """mi_so3n_laplacian: the connection Laplacian with the weights in force as a So3NCertificate (apply, apply_blocks;
        no null_panel); problem-owned in a slot of its own, refreshed by every call"""
        h = vp()
        check(self.L.mi_so3n_laplacian(self.h, C.byref(h)))
        return So3NCertificate(self, h)

    def lap_jacobi(self, k, X, Z=None):
        """mi_so3n_lap_jacobi: Z = X / degw row block by row block on column-major 3N x k panels (Z may be X)"""
        Z = Z if Z is not None else Vec(self.ctx, 3 * self.N * k)
        check(self.L.mi_so3n_lap_jacobi(self.h, k, X.h, Z.h))
        return Z

    def round(self, V, R=None, info=True):
        """mi_so3n_round: (R Vec of 9N, dict(negative, flipped, degenerate, min_separation)) from the column-major 3N x 3
        panel V; info=False: (R, None), no sync"""
        R = R if R is not None else Vec(self.ctx, 9 * self.N)
        out = np.zeros(4)
        check(self.L.mi_so3n_round(self.h, V.h, R.h, _dp(out) if info else None))
        return R, (dict(negative=int(out[0]), flipped=bool(out[1]), degenerate=int(out[2]), min_separation=out[3])
                   if info else None)

    def project(self, M, R=None, info=True):
        """mi_so3n_project: (R Vec of 9N, dict(defect, degenerate, negative)) from the 9N point M; R may be M"""
        R = R if R is not None else Vec(self.ctx, 9 * self.N)
        out = np.zeros(3)
        check(self.L.mi_so3n_project(self.h, M.h, R.h, _dp(out) if info else None))
        return R, (dict(defect=out[0], degenerate=int(out[1]), negative=int(out[2])) if info else None)

    ROBUST = {"l2": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3}

    def reweight(self, R, kind, c, info=True):
        """mi_so3n_reweight: w_e <- w0_e phi(|R_j - R_i Rt_e|_F; kind, c), kind a name of So3N.ROBUST or its number; R may
        be None for "l2".  info: dict(robust_cost, weighted_cost, outliers) from one read-back; info=False: None, no sync"""
        out = np.zeros(3)
        check(self.L.mi_so3n_reweight(self.h, R.h if R is not None else None, int(self.ROBUST.get(kind, kind)), float(c),
                                      _dp(out) if info else None))
        return dict(robust_cost=out[0], weighted_cost=out[1], outliers=int(out[2])) if info else None

    def weights(self):
        """mi_so3n_weights: the current edge weights (E doubles, the caller's edge order)"""
        w = np.zeros(self.E)
        check(self.L.mi_so3n_weights(self.h, _dp(w)))
        return w

    def armijo_trial(self, R, g, t, h=None, R_trial=None):
        """mi_so3n_armijo_trial: (h = -t g Vec, R_trial Vec, dict(f, grad_sqnorm))"""
        h = h if h is not None else Vec(self.ctx, 3 * self.N)
        Rt = R_trial if R_trial is not None else Vec(self.ctx, 9 * self.N)
        out = np.zeros(2)
        check(self.L.mi_so3n_armijo_trial(self.h, R.h, g.h, float(t), h.h, Rt.h, _dp(out)))
        return h, Rt, dict(f=out[0], grad_sqnorm=out[1])

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.L.mi_so3n_destroy(self.h)
        except Exception:  # noqa
            pass


class PgoTranslations:
    """The translation half of a pose graph (mi_pgo_trans_*): with the rotations R fixed, the positions solve
    L_a t = b(R) in the gauge t[anchor] = 0."""

    def __init__(self, ctx, N, ei, ej, tt, tau, anchor=0):
        self.ctx, self.L, self.N = ctx, ctx.L, N
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        ej = np.ascontiguousarray(ej, dtype=np.int32)
        tt = np.ascontiguousarray(tt, dtype=np.float64)
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        assert tt.size == 3 * ei.size and tau.size == ei.size and ej.size == ei.size
        self.E = ei.size
        self.h = vp()
        check(self.L.mi_pgo_trans_create(ctx.h, N, ei.size, ei.ctypes.data_as(c_int32_p), ej.ctypes.data_as(c_int32_p),
                                         _dp(tt), _dp(tau), int(anchor), C.byref(self.h)))

    def rhs(self, R, out=None):
        out = out if out is not None else Vec(self.ctx, 3 * self.N)
        check(self.L.mi_pgo_trans_rhs(self.h, R.h, out.h))
        return out

    def operator(self):
        """(L_a as an Op on 3N-vectors, its Jacobi Precon): borrowed, for Context.stpcg"""
        hop, pc = vp(), vp()
        check(self.L.mi_pgo_trans_operator(self.h, C.byref(hop), C.byref(pc)))
        P = Precon.__new__(Precon)
        P.ctx, P.L, P.h, P.keep = self.ctx, self.L, pc, [self]
        P.__class__ = _BorrowedPrecon
        return Op(self.ctx, hop, keep=[self], borrowed=True), P

    def residual(self, R, t, with_vector=True):
        """(r Vec of 3E or None, f_tau(R, t), max_e |r_e|): one read-back"""
        r = Vec(self.ctx, 3 * self.E) if with_vector else None
        out = (C.c_double * 2)()
        check(self.L.mi_pgo_trans_residual(self.h, R.h, t.h, r.h if with_vector else None, out))
        return r, out[0], out[1]

    def solve(self, R, tol=1e-10, max_iterations=1000, out=None):
        """(t Vec, dict(iterations, exit_reason, objective, relative_residual, max_residual))"""
        t = out if out is not None else Vec(self.ctx, 3 * self.N)
        info = PgoTransInfo()
        check(self.L.mi_pgo_trans_solve(self.h, R.h, float(tol), int(max_iterations), t.h, C.byref(info)))
        return t, dict(iterations=int(info.iterations), exit_reason=STPCG_EXIT[info.exit_reason],
                       objective=info.objective, relative_residual=info.relative_residual,
                       max_residual=info.max_residual)

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.L.mi_pgo_trans_destroy(self.h)
        except Exception:  # noqa
            pass


def _pgo_arrays(ei, ej, Rt, tt, kappa, tau):
    ei = np.ascontiguousarray(ei, dtype=np.int32)
    ej = np.ascontiguousarray(ej, dtype=np.int32)
    Rt, tt = np.ascontiguousarray(Rt, dtype=np.float64), np.ascontiguousarray(tt, dtype=np.float64)
    kappa, tau = np.ascontiguousarray(kappa, dtype=np.float64), np.ascontiguousarray(tau, dtype=np.float64)
    assert ej.size == ei.size and Rt.size == 9 * ei.size and tt.size == 3 * ei.size and kappa.size == tau.size == ei.size
    return ei, ej, Rt, tt, kappa, tau


PGO_PACK_ARRAYS = (("slice_ptr", np.int64), ("perm", np.int32), ("nbr", np.int32), ("slot", np.uint32), ("rinc", np.float64),
                   ("tinc", np.float64), ("kinc", np.float64), ("tauinc", np.float64))
PGO_PACK_COUNTS = ("N", "E", "nslices", "nnzb", "padded")


def pgo_pack(N, ei, ej, Rt, tt, kappa, tau):
    """mi_debug_pgo_pack (host only, no device): the layout of csrc/pgo_pack.h as dict(counts and arrays); a refused
    problem raises MiError with the packer's reason"""
    L = load()
    ei, ej, Rt, tt, kappa, tau = _pgo_arrays(ei, ej, Rt, tt, kappa, tau)
    args = (int(N), ei.size, ei.ctypes.data_as(c_int32_p), ej.ctypes.data_as(c_int32_p), _dp(Rt), _dp(tt), _dp(kappa), _dp(tau))
    k = len(PGO_PACK_ARRAYS)
    counts, n = (C.c_size_t * len(PGO_PACK_COUNTS))(), (C.c_size_t * k)()
    check(L.mi_debug_pgo_pack(*args, counts, None, None, n))          # the sizes
    arrays = [np.zeros(n[a], dtype=dtype) for a, (_, dtype) in enumerate(PGO_PACK_ARRAYS)]
    ptrs = (vp * k)(*[a.ctypes.data_as(vp) for a in arrays])
    check(L.mi_debug_pgo_pack(*args, counts, ptrs, (C.c_size_t * k)(*[a.size for a in arrays]), n))
    out = dict(zip(PGO_PACK_COUNTS, (int(c) for c in counts)))
    out.update({name: a for (name, _), a in zip(PGO_PACK_ARRAYS, arrays)})
    return out


class Pgo:
    """Joint pose-graph refinement on SE(3)^N (mi_pgo_*): point = 12N doubles [R | t], tangent = 6N doubles [xi_i, delta_i]."""

    def __init__(self, ctx, N, ei, ej, Rt, tt, kappa, tau):
        self.ctx, self.L, self.N = ctx, ctx.L, N
        ei, ej, Rt, tt, kappa, tau = _pgo_arrays(ei, ej, Rt, tt, kappa, tau)
        self.E = ei.size
        self.h = vp()
        check(self.L.mi_pgo_create(ctx.h, N, ei.size, ei.ctypes.data_as(c_int32_p), ej.ctypes.data_as(c_int32_p), _dp(Rt),
                                   _dp(tt), _dp(kappa), _dp(tau), C.byref(self.h)))

    def objective(self, x):
        f = C.c_double(0)
        check(self.L.mi_pgo_objective(self.h, x.h, C.byref(f)))
        return f.value

    def gradient(self, x, out=None):
        g = out if out is not None else Vec(self.ctx, 6 * self.N)
        check(self.L.mi_pgo_gradient(self.h, x.h, g.h))
        return g

    def model(self, x, with_precon=True):
        """(grad Vec, Hessian Op, block-Jacobi Precon or None), bound to x; the handles are the problem's"""
        g = Vec(self.ctx, 6 * self.N)
        hop, pc = vp(), vp()
        check(self.L.mi_pgo_model(self.h, x.h, g.h, C.byref(hop), C.byref(pc) if with_precon else None))
        P = None
        if with_precon:
            P = Precon.__new__(Precon)
            P.ctx, P.L, P.h, P.keep = self.ctx, self.L, pc, [self, x]
            P.__class__ = _BorrowedPrecon
        return g, Op(self.ctx, hop, keep=[self, x], borrowed=True), P

    def retract(self, x, eta):
        y = Vec(self.ctx, 12 * self.N)
        check(self.L.mi_pgo_retract(self.h, x.h, eta.h, y.h))
        return y

    def trial(self, x, h, g, with_precon=True):
        """mi_pgo_trial: (x_trial Vec, dict(f, hh, gh, hHh, grad_sqnorm, precon_grad_sqnorm))"""
        xt = Vec(self.ctx, 12 * self.N)
        out = np.zeros(6)
        check(self.L.mi_pgo_trial(self.h, x.h, h.h, g.h, int(with_precon), xt.h, _dp(out)))
        return xt, dict(f=out[0], hh=out[1], gh=out[2], hHh=out[3], grad_sqnorm=out[4], precon_grad_sqnorm=out[5])

    def hvp_dots(self, eta):
        """mi_debug_pgo_hvp_dots: (h = H eta Vec, (<eta,h>, <h,h>, <eta,eta>)) from one fused pass of the bound model"""
        h = Vec(self.ctx, 6 * self.N)
        out = np.zeros(3)
        check(self.L.mi_debug_pgo_hvp_dots(self.h, eta.h, h.h, _dp(out)))
        return h, tuple(out)

    BLOCKS = {"Bblk": 0, "Gblk": 1, "Nsl": 2, "Minv": 3, "Minv_trial": 4}

    def blocks(self, which):
        """mi_debug_pgo_blocks: one of Pgo.BLOCKS as the last model() (Minv_trial: the last trial()) wrote it"""
        n = C.c_size_t(0)
        check(self.L.mi_debug_pgo_blocks(self.h, self.BLOCKS[which], None, 0, C.byref(n), None))
        a = np.zeros(n.value)
        check(self.L.mi_debug_pgo_blocks(self.h, self.BLOCKS[which], _dp(a), a.size, C.byref(n), None))
        return a

    def info(self):
        """dict(nslices, nnzb, padded, model_grid)"""
        n, out = C.c_size_t(0), (C.c_size_t * 4)()
        check(self.L.mi_debug_pgo_blocks(self.h, 0, None, 0, C.byref(n), out))
        return dict(nslices=int(out[0]), nnzb=int(out[1]), padded=int(out[2]), model_grid=int(out[3]))

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.L.mi_pgo_destroy(self.h)
        except Exception:  # noqa
            pass


class So3NCertificate:
    """The certificate matrix S(R) of a So3N problem (mi_so3n_cert_*): borrowed from the problem, which it keeps alive."""

    def __init__(self, prob, h):
        self.prob, self.ctx, self.L, self.h, self.m = prob, prob.ctx, prob.L, h, 3 * prob.N

    def apply(self, k, X, Z=None):
        """mi_so3n_cert_apply: Z = S X on column-major 3N x k panels"""
        Z = Z if Z is not None else Vec(self.ctx, self.m * k)
        check(self.L.mi_so3n_cert_apply(self.h, k, X.h, Z.h))
        return Z

    def apply_blocks(self, blocks, Z=None):
        """mi_so3n_cert_apply_blocks: S [block 0 | block 1 | ...] for column blocks [(panel or view, columns), ...]"""
        k = sum(c for _, c in blocks)
        Z = Z if Z is not None else Vec(self.ctx, self.m * k)
        pb = PanelBlocks.of(blocks)
        check(self.L.mi_so3n_cert_apply_blocks(self.h, C.byref(pb), Z.h))
        return Z

    def null_panel(self):
        """mi_so3n_cert_null_panel: the 3N x 3 column-major panel Y, Y_i = R_i', as a borrowed Vec"""
        h = vp()
        check(self.L.mi_so3n_cert_null_panel(self.h, C.byref(h)))
        v = Vec(self.ctx, 0, handle=h)
        v.keep = self
        return v


class StiefelRQ:
    def __init__(self, ctx, A, n, p):
        self.ctx, self.L, self.A, self.n, self.p = ctx, ctx.L, A, n, p
        self.h = vp()
        check(self.L.mi_stiefel_rq_create(ctx.h, A.h, n, p, C.byref(self.h)))

    def objective(self, X):
        f = C.c_double(0)
        check(self.L.mi_stiefel_rq_objective(self.h, X.h, C.byref(f)))
        return f.value

    def model(self, X):
        """returns (grad Vec, Hessian Op bound to X)"""
        g = Vec(self.ctx, self.n * self.p)
        hop = vp()
        check(self.L.mi_stiefel_rq_model(self.h, X.h, g.h, C.byref(hop)))
        return g, Op(self.ctx, hop, keep=[self, X], borrowed=True)

    def trial(self, X, h, g):
        """mi_stiefel_rq_trial: (X_trial Vec, dict(f, hh, gh, hHh, grad_sqnorm))"""
        Xt = Vec(self.ctx, self.n * self.p)
        out = np.zeros(5)
        check(self.L.mi_stiefel_rq_trial(self.h, X.h, h.h, g.h, Xt.h, _dp(out)))
        return Xt, dict(f=out[0], hh=out[1], gh=out[2], hHh=out[3], grad_sqnorm=out[4])

    def precon(self, X, dinv_rows):
        h = vp()
        check(self.L.mi_stiefel_rq_precon(self.h, X.h, dinv_rows.h, C.byref(h)))
        return Precon(self.ctx, h, keep=[self, X, dinv_rows])

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.L.mi_stiefel_rq_destroy(self.h)
        except Exception:  # noqa
            pass
