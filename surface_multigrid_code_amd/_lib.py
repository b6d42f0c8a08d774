"""ctypes loader for lib/libsmg.so.  Fails loudly when the library is missing (no fallback path)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMG_LIB") or os.path.join(HERE, "lib", "libsmg.so")   # SMG_LIB: an alternate build (A/B measurements)

SMG_HOST, SMG_DEVICE = 0, 1


class SolveOptsC(C.Structure):
    _fields_ = [("tol", C.c_double), ("max_iter", C.c_int), ("pre", C.c_int), ("post", C.c_int),
                ("verbosity", C.c_int), ("check_every", C.c_int), ("use_graph", C.c_int), ("precision", C.c_int),
                ("smoother", C.c_int), ("omega", C.c_double), ("jacobi_max_rows", C.c_int), ("cheby_fraction", C.c_double)]


class MembraneParamsC(C.Structure):
    _fields_ = [("young", C.c_double), ("poisson", C.c_double), ("thickness", C.c_double), ("mass_scale", C.c_double), ("dt", C.c_double),
                ("pressure", C.c_double), ("newton_iters", C.c_int), ("ls_c", C.c_double), ("ls_shrink", C.c_double),
                ("ls_min_alpha", C.c_double), ("eig_floor", C.c_double), ("eig_value", C.c_double)]


class PdParamsC(C.Structure):
    _fields_ = [("dt", C.c_double), ("density", C.c_double), ("stiffness", C.c_double), ("sigma_min", C.c_double), ("sigma_max", C.c_double),
                ("pressure", C.c_double), ("gravity", C.c_double * 3)]


class DenoiseParamsC(C.Structure):
    _fields_ = [("sigma_s", C.c_double), ("sigma_r", C.c_double), ("fidelity", C.c_double), ("normal_iters", C.c_int)]


class StylizeParamsC(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("rho0", C.c_double), ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("mu", C.c_double),
                ("tau", C.c_double), ("admm_iters", C.c_int)]


class FlowParamsC(C.Structure):
    _fields_ = [("delta", C.c_double), ("normalize", C.c_int), ("stop_sphericity", C.c_double)]


class ConformalParamsC(C.Structure):
    _fields_ = [("grad_tol", C.c_double), ("max_newton", C.c_int), ("inner_rel_tol", C.c_double)]


class EmdParamsC(C.Structure):
    _fields_ = [("gap_tol", C.c_double), ("max_iter", C.c_int), ("check_every", C.c_int), ("alpha", C.c_double), ("rho_scale", C.c_double),
                ("inner_rel_tol", C.c_double)]


class FluidParamsC(C.Structure):
    _fields_ = [("theta", C.c_double), ("stages", C.c_int), ("viscosity", C.c_double), ("dt", C.c_double), ("cfl", C.c_double)]


class RdParamsC(C.Structure):
    _fields_ = [("Du", C.c_double), ("Dv", C.c_double), ("dt", C.c_double), ("react_substeps", C.c_int), ("stop_change", C.c_double)]


class WaveParamsC(C.Structure):
    _fields_ = [("dt", C.c_double), ("damping", C.c_double), ("clamped", C.c_int)]


_lib = None


# int reduce(double *d_sumsq, int count, void *hip_stream, void *ctx)   (include/smg.h: smg_reduce_fn)
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libsmg.so not built: run `python -m surface_multigrid_code_amd.build` "
                          "(expected at %s); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    ip, dp, vp, lp, fp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_float)
    i, d, f = C.c_int, C.c_double, C.c_float
    sig = {
        "smg_version": (i, []),
        "smg_last_error": (C.c_char_p, []),
        "smg_device_count": (i, []),
        "smg_device_bytes_live": (C.c_longlong, []),
        "smg_solve_opts_default": (None, [C.POINTER(SolveOptsC)]),
        "smg_hierarchy_create": (vp, [i]),
        "smg_hierarchy_destroy": (None, [vp]),
        "smg_hierarchy_levels": (i, [vp]),
        "smg_hierarchy_set_stream": (i, [vp, vp]),
        "smg_hierarchy_set_smoother": (i, [vp, i, d, i]),
        "smg_hierarchy_set_chebyshev": (i, [vp, d]),
        "smg_level_spectral_bound": (d, [vp, i]),
        "smg_level_set_prolong": (i, [vp, i, i, i, ip, ip, dp]),
        "smg_level_set_prolong_csc": (i, [vp, i, i, i, ip, ip, dp]),
        "smg_level_set_mesh": (i, [vp, i, dp, i, ip, i]),
        "smg_level_get_mesh": (i, [vp, i, ip, ip, dp, ip]),
        "smg_mg_precompute": (i, [dp, i, ip, i, f, i, i, C.POINTER(vp)]),
        "smg_mg_precompute_capped": (i, [dp, i, ip, i, f, i, i, f, C.POINTER(vp)]),
        "smg_mg_precompute_logged": (i, [dp, i, ip, i, f, i, i, f, i, C.POINTER(vp)]),
        "smg_query_coarse_to_fine": (i, [vp, i, i, ip, dp, ip, dp]),
        "smg_query_fine_to_coarse": (i, [vp, i, i, ip, dp, ip, dp]),
        "smg_mg_precompute_block": (i, [dp, i, ip, i, f, i, i, C.POINTER(vp)]),
        "smg_hierarchy_save": (i, [vp, C.c_char_p]),
        "smg_hierarchy_load": (i, [C.c_char_p, C.POINTER(vp)]),
        "smg_mg_precompute_subdiv": (i, [dp, i, ip, i, i, f, i, i, C.POINTER(vp), dp, ip]),
        "smg_precompute": (i, [vp, i, ip, ip, dp, ip, i]),
        "smg_precompute_values_device": (i, [vp, vp]),
        "smg_assembler_create": (i, [ip, i, i, C.POINTER(vp)]),
        "smg_assembler_destroy": (None, [vp]),
        "smg_assembler_pattern": (i, [vp, ip, ip, ip]),
        "smg_assemble": (i, [vp, vp, i, d, d, vp, vp, vp, vp]),
        "smg_solve": (i, [vp, vp, i, vp, i, vp, i, i, i, C.POINTER(SolveOptsC), vp, i, dp, ip, ip]),
        "smg_solve_pcg": (i, [vp, vp, i, vp, i, vp, i, i, i, C.POINTER(SolveOptsC), vp, i, dp, ip, ip]),
        "smg_eigs": (i, [vp, vp, i, i, vp, i, i, C.POINTER(SolveOptsC), C.c_ulonglong, dp, vp, i, dp, ip, ip]),
        "smg_debug_dense_geneig_host": (i, [i, dp, dp, dp, dp]),
        "smg_debug_eig_gram": (i, [i, i, i, dp, i, dp, dp, i, i, dp, ip, ip]),
        "smg_debug_eig_combine": (i, [i, i, i, dp, dp, dp, i, i, dp, dp, dp, dp, ip]),
        "smg_debug_eig_residual": (i, [i, i, dp, dp, dp, dp, i, i, dp, dp, fp, fp, dp, ip, ip]),
        "smg_debug_krylov": (i, [i, i, i, dp, dp, dp, dp, fp, dp, ip, d, i, dp, ip, ip, ip]),
        "smg_debug_cycle_f32": (i, [vp, i, i, i, i, i, i, fp, fp, fp, ip]),
        "smg_debug_convert_f32": (i, [vp, i, i, i, dp, fp, dp, fp, fp, ip]),
        "smg_debug_geodesics": (i, [i, i, i, i, ip, ip, ip, ip, ip, dp, dp, dp, dp, i, ip]),
        "smg_geodesics_create": (i, [vp, dp, i, ip, i, d, i, C.POINTER(vp)]),
        "smg_geodesics_destroy": (None, [vp]),
        "smg_geodesics_time": (d, [vp]),
        "smg_geodesics_set_solver": (i, [vp, i, i]),
        "smg_geodesics_device_bytes": (C.c_longlong, [vp]),
        "smg_geodesics_solve": (i, [vp, i, ip, ip, i, C.POINTER(SolveOptsC), C.POINTER(SolveOptsC), vp, i, ip]),
        "smg_debug_arap": (i, [i, i, ip, ip, dp, dp, dp, dp, dp, ip]),
        "smg_debug_fixed_reduce": (i, [i, i, dp, dp, ip, ip]),
        "smg_arap_create": (i, [vp, dp, i, ip, i, ip, i, C.POINTER(vp)]),
        "smg_arap_destroy": (None, [vp]),
        "smg_arap_set_solver": (i, [vp, i]),
        "smg_arap_device_bytes": (C.c_longlong, [vp]),
        "smg_arap_solve": (i, [vp, vp, i, vp, i, i, i, d, C.POINTER(SolveOptsC), vp, i, dp, ip, ip]),
        "smg_debug_membrane": (i, [i, i, i, ip, dp, dp, dp, C.POINTER(MembraneParamsC), dp, ip]),
        "smg_membrane_params_default": (None, [C.POINTER(MembraneParamsC)]),
        "smg_membrane_create": (i, [vp, dp, i, ip, i, C.POINTER(MembraneParamsC), C.POINTER(vp)]),
        "smg_membrane_destroy": (None, [vp]),
        "smg_membrane_device_bytes": (C.c_longlong, [vp]),
        "smg_membrane_set_state": (i, [vp, vp, vp, i]),
        "smg_membrane_get_state": (i, [vp, vp, vp, i]),
        "smg_membrane_set_solver": (i, [vp, i]),
        "smg_membrane_set_material": (i, [vp, i]),
        "smg_membrane_material": (i, [vp]),
        "smg_membrane_step": (i, [vp, C.POINTER(SolveOptsC), dp, dp, ip, ip]),
        "smg_membrane_lists": (i, [ip, i, i, ip, ip, ip, ip, ip, ip]),
        "smg_membrane_faces_host": (i, [dp, dp, i, ip, i, C.POINTER(MembraneParamsC), i, dp, dp, dp]),
        "smg_membrane_faces_host_material": (i, [dp, dp, i, ip, i, C.POINTER(MembraneParamsC), i, i, dp, dp, dp]),
        "smg_debug_membrane_material": (i, [i, i, i, i, ip, dp, dp, dp, C.POINTER(MembraneParamsC), dp, ip]),
        "smg_debug_param": (i, [i, i, i, ip, dp, dp, dp, dp, ip]),
        "smg_debug_union": (i, [i, i, i, i, ip, ip, dp, dp, dp, dp, ip, ip, dp, i, dp, C.POINTER(C.c_longlong), ip, ip, ip, dp, d, i, dp, ip, dp, ip]),
        "smg_param_create": (i, [vp, dp, i, ip, i, C.POINTER(vp)]),
        "smg_param_destroy": (None, [vp]),
        "smg_param_set_solver": (i, [vp, i]),
        "smg_param_device_bytes": (C.c_longlong, [vp]),
        "smg_param_boundary": (i, [vp, ip, ip]),
        "smg_param_harmonic": (i, [vp, i, C.POINTER(SolveOptsC), vp, i, ip]),
        "smg_param_arap": (i, [vp, vp, i, i, i, d, C.POINTER(SolveOptsC), vp, i, dp, ip, ip]),
        "smg_param_distortion": (i, [vp, vp, i, i, vp, dp]),
        "smg_pd_params_default": (None, [C.POINTER(PdParamsC)]),
        "smg_pd_create": (i, [vp, dp, i, ip, i, ip, i, C.POINTER(PdParamsC), C.POINTER(vp)]),
        "smg_pd_destroy": (None, [vp]),
        "smg_pd_device_bytes": (C.c_longlong, [vp]),
        "smg_pd_set_solver": (i, [vp, i]),
        "smg_pd_set_state": (i, [vp, vp, vp, i]),
        "smg_pd_get_state": (i, [vp, vp, vp, i]),
        "smg_pd_set_forces": (i, [vp, d, dp]),
        "smg_pd_set_strain_limits": (i, [vp, d, d]),
        "smg_pd_step": (i, [vp, vp, i, i, d, C.POINTER(SolveOptsC), dp, ip, ip]),
        "smg_pd_strain": (i, [vp, i, vp, dp]),
        "smg_pd_project_host": (i, [dp, dp, i, ip, i, d, d, dp, dp, dp, ip]),
        "smg_debug_pd": (i, [i, i, i, ip, dp, dp, dp, C.POINTER(PdParamsC), dp, ip]),
        "smg_denoise_params_default": (None, [C.POINTER(DenoiseParamsC)]),
        "smg_denoise_create": (i, [vp, dp, i, ip, i, C.POINTER(DenoiseParamsC), C.POINTER(vp)]),
        "smg_denoise_destroy": (None, [vp]),
        "smg_denoise_device_bytes": (C.c_longlong, [vp]),
        "smg_denoise_set_solver": (i, [vp, i]),
        "smg_denoise_sigma_s": (d, [vp]),
        "smg_denoise_set_filter": (i, [vp, d, d, i]),
        "smg_denoise_filter": (i, [vp, vp, i, vp]),
        "smg_denoise_update": (i, [vp, vp, i, i, d, C.POINTER(SolveOptsC), vp, dp, ip, ip]),
        "smg_denoise_run": (i, [vp, i, i, d, C.POINTER(SolveOptsC), vp, dp, ip, ip]),
        "smg_denoise_faces_host": (i, [i, i, i, ip, dp, dp, dp, C.POINTER(DenoiseParamsC), dp]),
        "smg_debug_denoise": (i, [i, i, i, ip, dp, dp, dp, C.POINTER(DenoiseParamsC), dp, ip]),
        "smg_stylize_params_default": (None, [C.POINTER(StylizeParamsC)]),
        "smg_stylize_create": (i, [vp, dp, i, ip, i, ip, i, C.POINTER(StylizeParamsC), C.POINTER(vp)]),
        "smg_stylize_destroy": (None, [vp]),
        "smg_stylize_device_bytes": (C.c_longlong, [vp]),
        "smg_stylize_set_solver": (i, [vp, i]),
        "smg_stylize_set_params": (i, [vp, C.POINTER(StylizeParamsC)]),
        "smg_stylize_set_lambda": (i, [vp, dp]),
        "smg_stylize_set_frame": (i, [vp, dp]),
        "smg_stylize_set_targets": (i, [vp, dp]),
        "smg_stylize_normals": (i, [vp, dp, dp]),
        "smg_stylize_run": (i, [vp, vp, i, vp, i, i, i, d, C.POINTER(SolveOptsC), vp, i, dp, ip, ip]),
        "smg_stylize_admm_stats": (i, [vp, ip, dp, ip, ip, ip]),
        "smg_stylize_local_host": (i, [i, i, i, ip, ip, ip, dp, dp, dp, dp, dp, dp, dp, dp, C.POINTER(StylizeParamsC), dp, ip]),
        "smg_debug_stylize": (i, [i, i, i, ip, ip, ip, dp, dp, dp, dp, dp, dp, dp, dp, C.POINTER(StylizeParamsC), dp, ip, ip]),
        "smg_morph_create": (i, [vp, dp, i, ip, i, ip, i, C.POINTER(vp)]),
        "smg_morph_destroy": (None, [vp]),
        "smg_morph_set_solver": (i, [vp, i]),
        "smg_morph_device_bytes": (C.c_longlong, [vp]),
        "smg_morph_reconstruct": (i, [vp, vp, i, vp, i, vp, i, i, C.POINTER(SolveOptsC), vp, i, ip]),
        "smg_morph_interpolate": (i, [vp, vp, dp, i, vp, i, vp, i, i, C.POINTER(SolveOptsC), vp, i, ip]),
        "smg_morph_transfer": (i, [vp, vp, i, ip, vp, i, vp, i, vp, i, i, C.POINTER(SolveOptsC), vp, i, ip]),
        "smg_morph_faces_host": (i, [i, i, i, i, ip, dp, dp, dp, dp, ip, i, dp]),
        "smg_debug_morph": (i, [i, i, i, i, ip, dp, dp, dp, dp, ip, i, dp, ip]),
        "smg_flow_params_default": (FlowParamsC, []),
        "smg_flow_create": (i, [vp, dp, i, ip, i, C.POINTER(FlowParamsC), C.POINTER(vp)]),
        "smg_flow_destroy": (None, [vp]),
        "smg_flow_set_params": (i, [vp, C.POINTER(FlowParamsC)]),
        "smg_flow_set_solver": (i, [vp, i]),
        "smg_flow_device_bytes": (C.c_longlong, [vp]),
        "smg_flow_step": (i, [vp, i, C.POINTER(SolveOptsC), dp, ip, ip]),
        "smg_flow_positions": (i, [vp, i, vp, i]),
        "smg_flow_set_positions": (i, [vp, vp, i, i]),
        "smg_flow_reset": (i, [vp]),
        "smg_flow_sphere": (i, [vp, i, vp, i, vp, dp]),
        "smg_flow_host": (i, [i, i, i, ip, dp, dp, ip, ip, dp, d, dp]),
        "smg_debug_flow": (i, [i, i, i, ip, dp, dp, ip, ip, dp, d, dp, ip]),
        "smg_hodge_create": (i, [vp, dp, i, ip, i, C.POINTER(vp)]),
        "smg_hodge_destroy": (None, [vp]),
        "smg_hodge_set_solver": (i, [vp, i]),
        "smg_hodge_is_closed": (i, [vp]),
        "smg_hodge_device_bytes": (C.c_longlong, [vp]),
        "smg_hodge_decompose": (i, [vp, vp, i, i, C.POINTER(SolveOptsC), vp, i, vp, i, vp, dp, ip]),
        "smg_hodge_field": (i, [vp, vp, i, vp, i, i, i, vp]),
        "smg_hodge_host": (i, [i, i, i, i, ip, dp, dp, dp, dp, dp]),
        "smg_debug_hodge": (i, [i, i, i, i, ip, dp, dp, dp, dp, dp, ip]),
        "smg_conformal_params_default": (ConformalParamsC, []),
        "smg_conformal_create": (i, [vp, dp, i, ip, i, ip, i, C.POINTER(ConformalParamsC), C.POINTER(vp)]),
        "smg_conformal_destroy": (None, [vp]),
        "smg_conformal_set_params": (i, [vp, C.POINTER(ConformalParamsC)]),
        "smg_conformal_set_solver": (i, [vp, i]),
        "smg_conformal_device_bytes": (C.c_longlong, [vp]),
        "smg_conformal_reset": (i, [vp]),
        "smg_conformal_set_u": (i, [vp, vp, i]),
        "smg_conformal_u": (i, [vp, i, vp]),
        "smg_conformal_solve": (i, [vp, vp, vp, i, C.POINTER(SolveOptsC), dp, dp, ip, ip, ip]),
        "smg_conformal_angle_sums": (i, [vp, i, vp]),
        "smg_conformal_lengths": (i, [vp, i, vp]),
        "smg_conformal_stats": (i, [vp, dp]),
        "smg_conformal_host": (i, [i, i, i, ip, dp, dp, dp, dp, d, dp, dp, ip, i, dp]),
        "smg_debug_conformal": (i, [i, i, i, ip, dp, dp, dp, dp, d, dp, dp, ip, i, dp, ip]),
        "smg_emd_params_default": (EmdParamsC, []),
        "smg_emd_create": (i, [vp, dp, i, ip, i, C.POINTER(EmdParamsC), C.POINTER(vp)]),
        "smg_emd_destroy": (None, [vp]),
        "smg_emd_set_params": (i, [vp, C.POINTER(EmdParamsC)]),
        "smg_emd_set_solver": (i, [vp, i]),
        "smg_emd_device_bytes": (C.c_longlong, [vp]),
        "smg_emd_solve": (i, [vp, vp, i, vp, i, i, i, C.POINTER(SolveOptsC), i, dp, dp, ip, dp, vp, i, vp]),
        "smg_emd_host": (i, [i, i, i, i, ip, dp, dp, dp, dp, dp, d, dp]),
        "smg_debug_emd": (i, [i, i, i, i, ip, dp, dp, dp, dp, dp, d, dp, ip]),
        "smg_fluid_params_default": (FluidParamsC, []),
        "smg_fluid_create": (i, [vp, dp, i, ip, i, C.POINTER(FluidParamsC), C.POINTER(vp)]),
        "smg_fluid_destroy": (None, [vp]),
        "smg_fluid_set_params": (i, [vp, C.POINTER(FluidParamsC)]),
        "smg_fluid_set_solver": (i, [vp, i]),
        "smg_fluid_is_closed": (i, [vp]),
        "smg_fluid_device_bytes": (C.c_longlong, [vp]),
        "smg_fluid_set_vorticity": (i, [vp, vp, i, i, i]),
        "smg_fluid_vorticity": (i, [vp, vp, i, i]),
        "smg_fluid_step": (i, [vp, i, C.POINTER(SolveOptsC), dp, dp, ip, ip]),
        "smg_fluid_stream": (i, [vp, C.POINTER(SolveOptsC), vp, i, i]),
        "smg_fluid_velocity": (i, [vp, C.POINTER(SolveOptsC), vp, i]),
        "smg_fluid_diagnostics": (i, [vp, C.POINTER(SolveOptsC), dp]),
        "smg_fluid_host": (i, [i, i, i, i, ip, dp, dp, dp, dp, d, d, dp, d, i, dp]),
        "smg_debug_fluid": (i, [i, i, i, i, ip, dp, dp, dp, dp, d, d, dp, d, i, dp, ip]),
        "smg_debug_fluid_time": (i, [i, i, i, i, ip, dp, i, i, dp]),
        "smg_rd_params_default": (RdParamsC, []),
        "smg_rd_create": (i, [vp, dp, i, ip, i, C.POINTER(RdParamsC), C.POINTER(vp)]),
        "smg_rd_destroy": (None, [vp]),
        "smg_rd_set_params": (i, [vp, C.POINTER(RdParamsC)]),
        "smg_rd_set_solver": (i, [vp, i]),
        "smg_rd_device_bytes": (C.c_longlong, [vp]),
        "smg_rd_set_state": (i, [vp, vp, vp, i, i, dp, i]),
        "smg_rd_state": (i, [vp, vp, vp, i, i]),
        "smg_rd_step": (i, [vp, i, C.POINTER(SolveOptsC), dp, dp, ip, ip]),
        "smg_rd_host": (i, [i, i, i, i, ip, dp, dp, dp, dp, d, i, dp, dp, dp]),
        "smg_debug_rd": (i, [i, i, i, i, ip, dp, dp, dp, dp, d, i, dp, dp, dp, ip]),
        "smg_debug_rd_time": (i, [i, i, i, i, ip, dp, i, i, dp]),
        "smg_sinkhorn_host": (i, [i, i, i, i, i, ip, dp, dp, dp, dp, dp, dp, dp, d, dp]),
        "smg_wave_params_default": (WaveParamsC, []),
        "smg_wave_create": (i, [vp, dp, i, ip, i, dp, dp, C.POINTER(WaveParamsC), C.POINTER(vp)]),
        "smg_wave_destroy": (None, [vp]),
        "smg_wave_set_params": (i, [vp, C.POINTER(WaveParamsC)]),
        "smg_wave_set_solver": (i, [vp, i]),
        "smg_wave_device_bytes": (C.c_longlong, [vp]),
        "smg_wave_set_state": (i, [vp, vp, vp, i, i, i]),
        "smg_wave_state": (i, [vp, vp, vp, i, i]),
        "smg_wave_set_sources": (i, [vp, ip, i]),
        "smg_wave_set_receivers": (i, [vp, ip, i]),
        "smg_wave_step": (i, [vp, i, dp, C.POINTER(SolveOptsC), dp, dp, ip, ip]),
        "smg_wave_host": (i, [i, i, i, i, ip, dp, dp, dp, i, d, dp, dp, dp, ip, i, dp, dp, dp]),
        "smg_debug_wave": (i, [i, i, i, i, ip, dp, dp, dp, i, d, dp, dp, dp, ip, i, dp, dp, dp, ip]),
        "smg_debug_wave_time": (i, [i, i, i, i, ip, dp, i, dp]),
        "smg_wave_gradient": (i, [vp, i, dp, dp, C.POINTER(SolveOptsC), dp, dp, i, dp, dp, i, dp, dp, ip, ip]),
        "smg_wave_set_speed": (i, [vp, dp]),
        "smg_wave_adjoint_host": (i, [i, i, i, i, ip, dp, dp, dp, i, d, dp, dp, dp, dp, dp, ip, i, i, dp]),
        "smg_debug_wave_adjoint": (i, [i, i, i, i, ip, dp, dp, dp, i, d, dp, dp, dp, dp, dp, ip, i, i, dp, ip]),
        "smg_wave_gauss_newton": (i, [vp, dp, i, i, C.POINTER(SolveOptsC), dp, i, dp, dp, ip]),
        "smg_wave_born_host": (i, [i, i, i, i, ip, i, dp, dp, dp, dp]),
        "smg_debug_wave_born": (i, [i, i, i, i, ip, i, dp, dp, dp, dp, ip]),
        "smg_solve_sharded": (i, [vp, vp, i, vp, i, vp, i, i, i, C.POINTER(SolveOptsC), REDUCE_FN, vp, vp, i, dp, ip, ip]),
        "smg_solve_begin": (i, [vp, vp, i, vp, i, vp, i, i, i, C.POINTER(SolveOptsC)]),
        "smg_solve_iter_residual": (i, [vp, vp]),
        "smg_solve_iter_cycle": (i, [vp, vp]),
        "smg_solve_iter_cycle_speculative": (i, [vp]),
        "smg_solve_iter_commit": (i, [vp, vp]),
        "smg_solve_poll": (i, [vp, ip, ip]),
        "smg_solve_end": (i, [vp, vp, i, i, dp, ip, ip]),
        "smg_level_rows": (i, [vp, i]),
        "smg_vcycle": (i, [vp, dp, i, i, i, dp, i]),
        "smg_apply_A": (i, [vp, i, dp, i, dp]),
        "smg_restrict": (i, [vp, i, dp, i, dp]),
        "smg_prolong": (i, [vp, i, dp, i, dp]),
        "smg_relax": (i, [vp, i, dp, i, i, dp]),
        "smg_coarse_solve": (i, [vp, dp, i, dp]),
        "smg_residual_norm": (i, [vp, i, dp, dp, i, dp]),
        "smg_raw_spmv": (i, [vp, i, i, vp, vp, vp, i]),
        "smg_raw_relax": (i, [vp, i, vp, vp, i, i]),
        "smg_raw_spmv_f32": (i, [vp, i, vp, vp, i]),
        "smg_raw_outer_iteration": (i, [vp, i]),
        "smg_synchronize": (i, [vp]),
        "smg_bench_vcycle": (i, [vp, i, i, i, i, i, dp]),
        "smg_bench_relax": (i, [vp, i, i, i, i, dp]),
        "smg_level_get_matrix": (i, [vp, i, i, i, ip, ip, ip, ip, ip, dp]),
        "smg_level_get_perm": (i, [vp, i, ip]),
        "smg_level_get_colors": (i, [vp, i, ip, ip]),
        "smg_level_get_Adiag": (i, [vp, i, dp]),
        "smg_get_unknown": (i, [vp, ip, ip]),
        "smg_level_sell_stats": (i, [vp, i, i, lp, lp, ip]),
        "smg_level_first_colour_rows": (i, [vp, i]),
        "smg_debug_check_tiling_plan": (i, [vp, i, i, i, ip, ip, dp, dp]),
        "smg_debug_check_sparse_cholesky": (i, [i, ip, ip, dp, lp, ip, dp]),
        "smg_hierarchy_set_coarse_dense_max": (i, [vp, i]),
        "smg_hierarchy_set_coarse_schur": (i, [vp, i, i]),
        "smg_debug_schur_solve_host": (i, [i, ip, ip, dp, dp, dp, ip, ip]),
        "smg_debug_schur_partition": (i, [vp, ip, ip, ip]),
        "smg_debug_wide_latency_variant": (i, [i, i]),
        "smg_debug_wgs_launches": (i, [i, i, i, i, ip, ip, ip, i, ip]),
        "smg_debug_wgs_level_plan": (i, [vp, i, i, i, ip, ip, ip]),
        "smg_debug_deep_launches": (i, [vp, i, i, i, i, ip, ip, i, ip]),
        "smg_debug_gs_colour_wpb": (i, [vp, i, i, ip, ip, ip]),
        "smg_hierarchy_set_block_gs": (i, [vp, i]),
        "smg_hierarchy_set_wave_gs": (i, [vp, i]),
        "smg_hierarchy_set_memory_lean": (i, [vp, i]),
        "smg_hierarchy_create_union": (i, [C.POINTER(vp), i, C.POINTER(vp)]),
        "smg_union_members": (i, [vp]),
        "smg_union_member_rows": (i, [vp, i, ip, ip]),
        "smg_union_get_history": (i, [vp, i, dp, i, ip, ip]),
        "smg_debug_device_bytes": (i, [vp, C.c_char_p, i]),
        "smg_level_get_wave_gs_order": (i, [vp, i, i, ip, ip, ip, ip, ip, dp]),
        "smg_debug_check_wave_gs_plan": (i, [vp, i, i, i, ip, ip, dp, dp]),
        "smg_debug_check_plan_value_maps": (i, [vp, i, i, i, i, ip, ip, ip, ip]),
        "smg_debug_raise_coarse_stall": (i, [vp]),
        "smg_debug_check_block_gs_plan": (i, [vp, i, i, ip, ip, dp, dp, dp]),
        "smg_level_get_block_gs_order": (i, [vp, i, i, ip, ip, ip, ip, ip, dp]),
        "smg_hierarchy_coarse_solver": (i, [vp, lp]),
        "smg_hierarchy_set_block_mode": (i, [vp, i]),
        "smg_hierarchy_block_size": (i, [vp]),
        "smg_level_block_stats": (i, [vp, i, lp, lp, ip]),
        "smg_level_get_block_image": (i, [vp, i, ip, ip, ip, ip, ip, ip, dp]),
        "smg_level_spmv_bytes": (C.c_long, [vp, i, i]),
        "smg_vcycle_bytes": (C.c_long, [vp, i, i, i]),
        "smg_prof_enable": (i, [vp, i]),
        "smg_prof_reset": (i, [vp]),
        "smg_prof_count": (i, [vp]),
        "smg_prof_get": (i, [vp, i, C.c_char_p, i, lp, dp]),
        "smg_mesh_read": (i, [C.c_char_p, C.POINTER(dp), ip, C.POINTER(ip), ip]),
        "smg_free": (None, [vp]),
        "smg_mesh_normalize_unit_area": (i, [dp, i, ip, i]),
        "smg_mesh_cotmatrix": (i, [dp, i, ip, i, ip, ip, ip, dp]),
        "smg_mesh_massmatrix": (i, [dp, i, ip, i, i, dp]),
        "smg_mesh_boundary_loop": (i, [ip, i, i, ip, ip]),
        "smg_mesh_face_neighbours": (i, [ip, i, i, ip, ip]),
        "smg_mesh_unfold": (i, [ip, i, i, dp, dp, dp]),
        "smg_mesh_midpoint_upsample": (i, [i, ip, i, ip, ip, ip, dp, ip]),
        "smg_mesh_torus": (i, [i, i, d, d, dp, ip]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError here = the library does not export what smg.h declares
        fn.restype = res
        fn.argtypes = args
    L._smg_signatures = sig
    _lib = L
    return L


def exported_symbols():
    """Every entry point include/smg.h declares (used by the CPU-side ABI test)."""
    return sorted(load()._smg_signatures.keys())
