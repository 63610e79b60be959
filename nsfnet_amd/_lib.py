"""ctypes binding of include/nsfnet_pinn.h.  The HIP library IS the product path:
there is no CPU or torch fallback - loading fails loudly when it is missing."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# $NSFNET_PINN_LIB selects another build of the same ABI (kernel experiments: scripts/abl_build.py)
LIB_PATH = os.environ.get("NSFNET_PINN_LIB") or os.path.join(_HERE, "lib", "libnsfnet_pinn.so")

c_void_p, c_int, c_int64, c_float, c_double = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double

# name -> (restype, argtypes); mirrors include/nsfnet_pinn.h one to one
SIGNATURES = {
    "pinn_last_error": (ctypes.c_char_p, []),
    "pinn_abi_version": (c_int, []),
    "pinn_net_create": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "pinn_net_destroy": (c_int, [c_void_p]),
    "pinn_net_set_precision": (c_int, [c_void_p, c_int, c_int, c_int]),
    "pinn_net_set_first_layer": (c_int, [c_void_p, c_int]),
    "pinn_net_first_layer": (c_int, [c_void_p]),
    "pinn_net_num_params": (c_int64, [c_void_p]),
    "pinn_net_prep_floats": (c_int64, [c_void_p]),
    "pinn_net_prepare": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_plan_create": (c_int, [c_void_p, c_int64, c_int, ctypes.POINTER(c_void_p)]),
    "pinn_plan_destroy": (c_int, [c_void_p]),
    "pinn_plan_padded_points": (c_int64, [c_void_p]),
    "pinn_plan_workspace_bytes": (c_int64, [c_void_p, c_int]),
    "pinn_plan_kernel": (ctypes.c_char_p, [c_void_p, c_int]),
    "pinn_residual_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                                      c_int, c_void_p, c_void_p]),
    "pinn_residual_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, ctypes.POINTER(c_float), c_float, c_float,
                                       c_void_p, c_void_p]),
    "pinn_residual_backward_phases": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, ctypes.POINTER(c_float), c_float, c_float,
                                              c_void_p, c_int, c_void_p]),
    "pinn_residual_forward_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_float), c_float, c_float,
                                               c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "pinn_value_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_float),
                                   c_int, c_void_p, c_void_p]),
    "pinn_value_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_grad_reduce": (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p),
                                 c_void_p, c_int, c_void_p]),
    "pinn_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                               c_float, c_float, c_float, c_float, c_int64, c_void_p]),
    "pinn_adam_step_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                   c_float, c_float, c_float, c_float, c_void_p, c_void_p]),
    "pinn_resample_scratch_bytes": (c_int64, [c_int64]),
    "pinn_resample_select": (c_int, [c_int64, c_void_p, c_int64, c_double, c_double, c_double, c_double, c_int64,
                                     c_void_p, c_void_p, c_void_p]),
    "pinn_resample_gather": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_lbfgs_workspace_bytes": (c_int64, [c_int64, c_int]),
    "pinn_lbfgs_reset": (c_int, [c_void_p, c_int64, c_int, c_void_p]),
    "pinn_lbfgs_direction": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "pinn_lbfgs_probe": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_balance_partials_count": (c_int64, [c_int64]),
    "pinn_grad_reduce_terms": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_void_p),
                                       ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_void_p, c_void_p]),
    "pinn_balance_stats": (c_int, [ctypes.POINTER(c_void_p), c_int64, c_void_p, c_void_p]),
    "pinn_balance_update": (c_int, [c_void_p, c_int64, c_int, c_double, c_void_p, c_void_p, c_void_p]),
    "pinn_balance_combine": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "pinn_confgrad_partials_count": (c_int64, [c_int64]),
    "pinn_grad_reduce_terms_gram": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_void_p),
                                            ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_void_p, c_void_p,
                                            c_void_p]),
    "pinn_confgrad_gram": (c_int, [ctypes.POINTER(c_void_p), c_int64, c_void_p, c_void_p]),
    "pinn_confgrad_coef": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "pinn_confgrad_combine": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "pinn_batch_draw": (c_int, [c_int64, c_int64, ctypes.c_uint64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_batch_scatter": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "pinn_rba_scratch_bytes": (c_int64, [c_int64]),
    "pinn_rba_stats": (c_int, [c_int64, c_void_p, c_int64, c_double, c_void_p, c_void_p]),
    "pinn_rba_apply": (c_int, [c_int64, c_void_p, c_int64, c_double, c_double, c_double, c_void_p, c_int64, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_rba_fill": (c_int, [c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_val_scratch_bytes": (c_int64, []),
    "pinn_val_stats": (c_int, [c_int64, c_void_p, c_void_p, c_int, c_double, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                               c_void_p]),
    "pinn_val_keep": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "pinn_flow_scratch_bytes": (c_int64, []),
    "pinn_flow_stream_function": (c_int, [c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "pinn_flow_stats": (c_int, [c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_double, c_double,
                                c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "pinn_plan_create_constrained": (c_int, [c_void_p, c_int64, c_int, c_void_p, ctypes.POINTER(c_void_p)]),
    "pinn_plan_hard_bc": (c_int, [c_void_p, c_void_p]),
    "pinn_lr_schedule_value": (c_double, [c_void_p, c_double, c_int64]),
    "pinn_grad_sqnorm_scratch_bytes": (c_int64, []),
    "pinn_grad_sqnorm": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "pinn_adam_step_sched": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_double, c_float, c_float,
                                     c_float, c_void_p, c_void_p, c_int, c_void_p, c_double, c_void_p, c_void_p]),
    "pinn_rwf_rows": (c_int64, [c_void_p]),
    "pinn_rwf_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_rwf_compose": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_rwf_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_plan_create_pseudo_time": (c_int, [c_void_p, c_int64, c_void_p, ctypes.POINTER(c_void_p)]),
    "pinn_plan_set_pseudo_time": (c_int, [c_void_p, c_void_p, c_float, c_float]),
    "pinn_plan_pseudo_time": (c_int, [c_void_p, ctypes.POINTER(c_float), ctypes.POINTER(c_float)]),
    "pinn_ptime_scratch_bytes": (c_int64, [c_int64]),
    "pinn_ptime_advance": (c_int, [c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p,
                                   c_void_p]),
    "pinn_monitor_scratch_bytes": (c_int64, []),
    "pinn_monitor_vis_stats": (c_int, [c_int64, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_monitor_observe": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_double, c_double, c_double,
                                     c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_plan_set_viscosity": (c_int, [c_void_p, c_void_p, c_void_p]),
    "pinn_plan_viscosity": (c_int, [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p)]),
    "pinn_visc_scratch_bytes": (c_int64, [c_int64]),
    "pinn_visc_grad": (c_int, [c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p]),
    "pinn_visc_update": (c_int, [c_void_p, c_double, c_double, c_double, c_double, c_double, c_double, c_double, c_void_p,
                                 c_void_p, c_void_p]),
    "pinn_plan_set_viscosity_cap": (c_int, [c_void_p, c_void_p]),
    "pinn_plan_viscosity_cap": (c_int, [c_void_p, ctypes.POINTER(c_void_p)]),
    "pinn_visc_schedule_value": (c_double, [c_void_p, c_int64, c_void_p]),
    "pinn_visc_schedule_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_state_scratch_bytes": (c_int64, []),
    "pinn_state_layout": (c_int64, [c_int, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "pinn_state_digest_host": (c_int, [c_void_p, c_int64, ctypes.POINTER(ctypes.c_uint64)]),
    "pinn_state_pack": (c_int, [c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64), ctypes.POINTER(c_int64), c_void_p,
                                c_int64, c_void_p, c_void_p, c_void_p]),
    "pinn_state_unpack": (c_int, [c_int, c_void_p, c_int64, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64),
                                  ctypes.POINTER(c_void_p), c_void_p, c_void_p, c_void_p]),
}


class LrScheduleStruct(ctypes.Structure):
    """pinn_lr_schedule_t"""
    _fields_ = [("kind", ctypes.c_int32), ("n_milestones", ctypes.c_int32), ("milestones", c_int64 * 16),
                ("step_size", c_int64), ("t_max", c_int64), ("warmup_epochs", c_int64),
                ("gamma", c_double), ("eta_min", c_double), ("warmup_start", c_double)]


class HardBcStruct(ctypes.Structure):
    """pinn_hard_bc_t"""
    _fields_ = [("kind", ctypes.c_int32), ("lift_power", ctypes.c_int32), ("x0", c_float), ("y0", c_float),
                ("inv_len", c_float), ("lid_sharpness", c_float)]


class ViscScheduleStruct(ctypes.Structure):
    """pinn_visc_schedule_t"""
    _fields_ = [("shape", ctypes.c_int32), ("stairs", ctypes.c_int32), ("hold", c_int64), ("updates", c_int64),
                ("re_start", c_double), ("re_end", c_double), ("cap_factor", c_double), ("nu_start", c_float),
                ("nu_end", c_float), ("cap_start", c_float), ("cap_end", c_float)]


class MonitorConfigStruct(ctypes.Structure):
    """pinn_monitor_config_t"""
    _fields_ = [("every", c_int64), ("window", c_int64), ("patience", c_int64), ("min_updates", c_int64),
                ("capacity", c_int64), ("quantity", ctypes.c_int32), ("ev", ctypes.c_int32), ("plateau_on", ctypes.c_int32),
                ("re_eff_on", ctypes.c_int32), ("min_rel_improvement", c_double), ("re_eff_tol", c_double)]


_lib = None


class PinnLibraryError(RuntimeError):
    pass


def load():
    """Load libnsfnet_pinn.so (built by nsfnet_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PinnLibraryError(
            "HIP library %s is missing - build it with `python -m nsfnet_amd.build`; "
            "there is no CPU fallback for the PINN hot path" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the .so does not export it
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().pinn_last_error()
        raise PinnLibraryError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
