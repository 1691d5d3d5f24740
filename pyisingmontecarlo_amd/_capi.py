"""ctypes binding of include/isingmc.h (libisingmc.so).  No fallback of any kind: if the HIP library
is missing or no device is usable, calls raise."""
import ctypes as C
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ISINGMC_LIB_PATH") or os.path.join(_HERE, "lib", "libisingmc.so")  # override: A/B builds

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_ALLOC = range(5)
KIND_GENERAL, KIND_LATTICE2D = 0, 1
FLAG_FORCE_GENERAL = 1
FLAG_STABLE_PATH = 2
MOMENTS_PER_REPLICA = 1  # ISINGMC_MOMENTS_*
MOMENTS_BONDS = 2
MOMENTS_PER_RUNG = 4
SERIES_LINK = 1  # ISINGMC_SERIES_*
SERIES_BY_RUNG = 2
OBS_ENERGY = 1  # ISINGMC_OBS_*
OBS_MAGNETISATION = 2
OBS_BY_RUNG = 4
FAMILIES = ("checkerboard", "csr_f64", "packed_bitsliced", "packed_real")


class GraphInfo(C.Structure):
    _fields_ = [("kind", C.c_int32), ("device", C.c_int32), ("nvars", C.c_uint64), ("n_edges", C.c_uint64),
                ("width", C.c_int32), ("height", C.c_int32), ("jabs", C.c_double), ("uniform_sign", C.c_int32),
                ("n_colours", C.c_uint32), ("state_words", C.c_uint64), ("fast_path", C.c_int32), ("open_x", C.c_int32),
                ("open_y", C.c_int32), ("field", C.c_double), ("jabs_y", C.c_double),
                ("field_signs", C.c_int32), ("packed_degree", C.c_int32), ("real_slots", C.c_int32),
                ("real_quantum_log2", C.c_int32), ("real_energy_log2", C.c_int32), ("real_heavy_sites", C.c_int32),
                ("stable_path", C.c_int32), ("packed_but_one_headers", C.c_int32)]


_vp = C.c_void_p
_PROTOTYPES = {
    "isingmc_last_error": (C.c_char_p, []),
    "isingmc_abi_version": (C.c_int, []),
    "isingmc_release_cached_resources": (C.c_size_t, []),
    "isingmc_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "isingmc_host_make_seeds": (C.c_int, [C.c_int, C.c_uint64, C.c_size_t, _vp]),
    "isingmc_host_expand_schedule": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_int, _vp]),
    "isingmc_host_recognise_lattice2d": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_int),
                                                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                                   C.POINTER(C.c_int)]),
    "isingmc_host_colour_graph": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, C.POINTER(C.c_uint32)]),
    "isingmc_host_pt_swap_round": (C.c_int, [C.c_uint64, C.c_uint64, C.c_size_t, _vp, _vp, _vp,
                                             C.POINTER(C.c_uint64)]),
    "isingmc_host_pt_statistics_round": (C.c_int, [C.c_uint64, C.c_size_t] + [_vp] * 11 + [C.POINTER(C.c_uint64)]),
    "isingmc_host_pa_sources": (C.c_int, [C.c_uint64, C.c_uint64, C.c_size_t, _vp, C.c_double, _vp, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_double)]),
    "isingmc_host_pa_choose_step": (C.c_int, [C.c_size_t, _vp, C.c_double, C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_double),
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "isingmc_host_class_segments": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, C.POINTER(C.c_size_t), _vp,
                                              C.POINTER(C.c_size_t), _vp]),
    "isingmc_host_rj_quantise": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp, C.POINTER(C.c_int),
                                           C.POINTER(C.c_int)]),
    "isingmc_host_rj_energy_levels": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int)]),
    "isingmc_host_rj_beta": (C.c_int, [C.c_double, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "isingmc_host_rj_log_table": (C.c_int, [_vp]),
    "isingmc_graph_create": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_int, C.c_uint, C.POINTER(_vp)]),
    "isingmc_graph_info": (C.c_int, [_vp, C.POINTER(GraphInfo)]),
    "isingmc_graph_destroy": (None, [_vp]),
    "isingmc_states_create": (C.c_int, [_vp, C.c_size_t, _vp, _vp, C.POINTER(_vp)]),
    "isingmc_states_create_range": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, C.POINTER(_vp)]),
    "isingmc_states_append": (C.c_int, [_vp, C.c_uint64, _vp]),
    "isingmc_states_set_state": (C.c_int, [_vp, C.c_size_t, _vp]),
    "isingmc_states_count": (C.c_size_t, [_vp]),
    "isingmc_states_destroy": (None, [_vp]),
    "isingmc_graph_family_for": (C.c_int, [_vp, C.c_size_t, C.POINTER(C.c_int)]),
    "isingmc_states_family": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "isingmc_states_set_option": (C.c_int, [_vp, C.c_char_p, C.c_long]),
    "isingmc_states_philox_rounds": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "isingmc_graph_philox_rounds": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "isingmc_states_set_betas": (C.c_int, [_vp, _vp]),
    "isingmc_do_time_steps": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "isingmc_do_time_steps_timed": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_float)]),
    "isingmc_get_energies": (C.c_int, [_vp, _vp]),
    "isingmc_get_magnetisations": (C.c_int, [_vp, _vp]),
    "isingmc_get_states": (C.c_int, [_vp, _vp, C.c_size_t]),
    "isingmc_get_packed_states": (C.c_int, [_vp, _vp]),
    "isingmc_get_raw_state": (C.c_int, [_vp, _vp, C.POINTER(C.c_size_t)]),
    "isingmc_states_timestep": (C.c_uint64, [_vp]),
    "isingmc_states_set_timestep": (C.c_int, [_vp, C.c_uint64]),
    "isingmc_states_set_cluster_every": (C.c_int, [_vp, C.c_size_t]),
    "isingmc_states_cluster_every": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "isingmc_cluster_stats": (C.c_int, [_vp, _vp, _vp]),
    "isingmc_states_set_icm_every": (C.c_int, [_vp, C.c_size_t]),
    "isingmc_states_icm_every": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "isingmc_icm_stats": (C.c_int, [_vp, _vp, _vp, _vp]),
    "isingmc_icm_between": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t]),
    "isingmc_icm_between_stats": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t]),
    "isingmc_overlaps": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "isingmc_site_classes_create": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.POINTER(_vp)]),
    "isingmc_site_classes_destroy": (C.c_int, [_vp]),
    "isingmc_site_classes_sizes": (C.c_int, [_vp, _vp]),
    "isingmc_overlaps_by_class": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "isingmc_overlap_series_create": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_uint, C.c_size_t, C.POINTER(_vp)]),
    "isingmc_overlap_series_record": (C.c_int, [_vp, _vp, _vp]),
    "isingmc_overlap_series_set_every": (C.c_int, [_vp, C.c_size_t]),
    "isingmc_overlap_series_count": (C.c_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "isingmc_overlap_series_get": (C.c_int, [_vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp]),
    "isingmc_overlap_series_reset": (C.c_int, [_vp]),
    "isingmc_overlap_series_destroy": (C.c_int, [_vp]),
    "isingmc_observable_series_create": (C.c_int, [_vp, _vp, C.c_uint, C.c_size_t, C.POINTER(_vp)]),
    "isingmc_observable_series_record": (C.c_int, [_vp]),
    "isingmc_observable_series_set_every": (C.c_int, [_vp, C.c_size_t]),
    "isingmc_observable_series_count": (C.c_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "isingmc_observable_series_get": (C.c_int, [_vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp]),
    "isingmc_observable_series_reset": (C.c_int, [_vp]),
    "isingmc_observable_series_destroy": (C.c_int, [_vp]),
    "isingmc_host_nonlocal_steps": (C.c_int, [C.c_uint64, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)]),
    "isingmc_states_set_track_best": (C.c_int, [_vp, C.c_size_t]),
    "isingmc_states_track_best": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "isingmc_best_update": (C.c_int, [_vp]),
    "isingmc_best_get": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.POINTER(C.c_uint64)]),
    "isingmc_best_raw_state": (C.c_int, [_vp, _vp, C.POINTER(C.c_size_t)]),
    "isingmc_best_reset": (C.c_int, [_vp]),
    "isingmc_states_set_moments_every": (C.c_int, [_vp, C.c_size_t, C.c_uint]),
    "isingmc_states_moments_every": (C.c_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint)]),
    "isingmc_moments_accumulate": (C.c_int, [_vp]),
    "isingmc_moments_get": (C.c_int, [_vp, C.POINTER(C.c_uint64), _vp, _vp]),
    "isingmc_moments_reset": (C.c_int, [_vp]),
    "isingmc_run_sampling_moments": (C.c_int, [_vp, C.c_double, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, _vp]),
    "isingmc_autocorr_create": (C.c_int, [_vp, C.c_size_t, C.c_uint, C.POINTER(_vp)]),
    "isingmc_autocorr_set_every": (C.c_int, [_vp, C.c_size_t]),
    "isingmc_autocorr_sample": (C.c_int, [_vp]),
    "isingmc_autocorr_count": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]),
    "isingmc_autocorr_get": (C.c_int, [_vp, _vp, _vp]),
    "isingmc_autocorr_reset": (C.c_int, [_vp]),
    "isingmc_autocorr_destroy": (C.c_int, [_vp]),
    "isingmc_run_sampling_autocorr": (C.c_int, [_vp, C.c_double, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _vp]),
    "isingmc_host_autocorr_plan": (C.c_int, [C.c_uint64, C.c_size_t, _vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _vp]),
    "isingmc_run_sampling": (C.c_int, [_vp, C.c_double, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp]),
    "isingmc_pt_attach": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint64]),
    "isingmc_pt_can_attach": (C.c_int, [_vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_int)]),
    "isingmc_pt_detach": (C.c_int, [_vp]),
    "isingmc_pt_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "isingmc_pt_group_create": (C.c_int, [_vp, C.c_size_t, C.c_int, C.POINTER(_vp)]),
    "isingmc_pt_group_backend": (C.c_int, [_vp]),
    "isingmc_pt_group_allgather": (C.c_int, [_vp]),
    "isingmc_pt_group_run": (C.c_int, [_vp, C.c_size_t, C.c_size_t]),
    "isingmc_pt_group_synchronize": (C.c_int, [_vp]),
    "isingmc_pt_group_destroy": (None, [_vp]),
    "isingmc_pt_time_steps": (C.c_int, [_vp, C.c_size_t]),
    "isingmc_pt_measure": (C.c_int, [_vp]),
    "isingmc_pt_run": (C.c_int, [_vp, C.c_size_t, C.c_size_t]),
    "isingmc_pt_swap": (C.c_int, [_vp]),
    "isingmc_pt_state": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "isingmc_pt_set_statistics": (C.c_int, [_vp, C.c_int]),
    "isingmc_pt_statistics_get": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)] + [_vp] * 8),
    "isingmc_pt_statistics_reset": (C.c_int, [_vp]),
    "isingmc_pa_resample": (C.c_int, [_vp, C.c_double, C.c_uint64, C.c_uint64]),
    "isingmc_pa_apply_sources": (C.c_int, [_vp, _vp]),
    "isingmc_pa_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_uint64, _vp, _vp, _vp, _vp]),
    "isingmc_pa_choose_step": (C.c_int, [_vp, C.c_double, C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "isingmc_pa_run_adaptive": (C.c_int, [_vp, C.c_double, C.c_double, C.c_size_t, C.c_uint64, C.c_double, C.c_double, C.c_size_t, _vp,
                                          C.POINTER(C.c_size_t), _vp, _vp, _vp, _vp]),
    "isingmc_pa_last": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "isingmc_pa_families": (C.c_int, [_vp, _vp]),
    "isingmc_pa_reset_families": (C.c_int, [_vp]),
    "isingmc_states_stream": (C.c_int, [_vp, C.POINTER(_vp)]),
    "isingmc_synchronize": (C.c_int, [_vp]),
    "isingmc_debug_shader_clock": (C.c_int, [_vp, C.c_size_t, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "isingmc_debug_live_blocks": (C.c_int, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
}
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)
# include/isingmc_cluster_series.h: the header isingmc.h includes at its end, bound with the table above
_CLUSTER_SERIES_PROTOTYPES = {
    "isingmc_cluster_series_create": (C.c_int, [_vp, C.c_int, C.c_size_t, C.POINTER(_vp)]),
    "isingmc_cluster_series_count": (C.c_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "isingmc_cluster_series_get": (C.c_int, [_vp, C.c_size_t, C.c_size_t, _vp, _vp]),
    "isingmc_cluster_series_reset": (C.c_int, [_vp]),
    "isingmc_cluster_series_destroy": (C.c_int, [_vp]),
}
CLUSTER_SERIES_SYMBOLS = tuple(_CLUSTER_SERIES_PROTOTYPES)

_lib = None
_hip_preloaded = False


def preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  Whichever copy a
    process loads first serves both torch and libisingmc.so; if the system copy wins, torch's other bundled
    ROCm libraries no longer match it and torch.cuda reports no GPU.  So when torch is installed its copy
    is loaded first (without importing torch); libisingmc.so then binds to that one."""
    global _hip_preloaded
    if _hip_preloaded:
        return
    _hip_preloaded = True
    if os.environ.get("ISINGMC_NO_TORCH_HIP_PRELOAD"):  # diagnostics: run on the system ROCm runtime
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:  # pragma: no cover - torch absent or laid out differently: use the system runtime
        pass


def lib():
    global _lib
    if _lib is None:
        preload_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m pyisingmontecarlo_amd.build` "
                "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(_PROTOTYPES.items()) + list(_CLUSTER_SERIES_PROTOTYPES.items()):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.isingmc_abi_version() != 4:
            raise RuntimeError("libisingmc.so ABI version mismatch")
        _lib = L
    return _lib


def _check(rc):
    if rc == OK:
        return
    msg = (lib().isingmc_last_error() or b"").decode()
    if rc == ERR_INVALID:
        raise ValueError(msg)
    if rc == ERR_ALLOC:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def last_error():
    return (lib().isingmc_last_error() or b"").decode()


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _arr(x, dtype):
    return None if x is None else np.ascontiguousarray(x, dtype=dtype)


def device_count():
    n = C.c_int(0)
    rc = lib().isingmc_device_count(C.byref(n))
    return n.value if rc == OK else 0


def make_seeds(seed_gen, n):
    out = np.zeros(n, dtype=np.uint64)
    _check(lib().isingmc_host_make_seeds(int(seed_gen is not None), C.c_uint64(seed_gen or 0), n, _p(out)))
    return out


def expand_schedule(stops, timesteps, compat_constant_beta=False):
    t = _arr([s[0] for s in stops], np.uint64)
    b = _arr([s[1] for s in stops], np.float64)
    out = np.zeros(timesteps, dtype=np.float64)
    _check(lib().isingmc_host_expand_schedule(_p(t), _p(b), len(stops), timesteps, int(compat_constant_beta), _p(out)))
    return out


def recognise_lattice2d(ea, eb, ej, nvars):
    ea, eb, ej = _arr(ea, np.uint64), _arr(eb, np.uint64), _arr(ej, np.float64)
    ok, w, h, u, jabs = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
    _check(lib().isingmc_host_recognise_lattice2d(_p(ea), _p(eb), _p(ej), len(ea), nvars, C.byref(ok), C.byref(w),
                                                  C.byref(h), C.byref(jabs), C.byref(u)))
    out = dict(is_lattice=bool(ok.value), width=w.value, height=h.value, jabs=jabs.value, uniform_sign=bool(u.value))
    if ok.value > 0 and (ok.value - 1) & 6:  # open boundaries (all wrap-around bonds of a direction absent)
        out.update(open_x=bool((ok.value - 1) & 2), open_y=bool((ok.value - 1) & 4))
    if ok.value > 0 and (ok.value - 1) & 8:  # jabs is the horizontal bonds' |J|, the vertical bonds have another
        out.update(anisotropic=True)
    return out


def rj_quantise(ea, eb, ej, nvars, biases=None):
    """(k, jq[n_edges, 2] (each bond as seen from its two ends), hq per site, dshift per site, eligible) of the real-coupling
    packed path."""
    ea, eb, ej, b = _arr(ea, np.uint64), _arr(eb, np.uint64), _arr(ej, np.float64), _arr(biases, np.float64)
    jq, hq, d = np.zeros((len(ea), 2), dtype=np.int32), np.zeros(nvars, dtype=np.int32), np.zeros(nvars, dtype=np.uint8)
    k, ok = C.c_int(), C.c_int()
    _check(lib().isingmc_host_rj_quantise(_p(ea), _p(eb), _p(ej), len(ea), nvars, _p(b), _p(jq), _p(hq), _p(d), C.byref(k), C.byref(ok)))
    return k.value, jq, hq, d, bool(ok.value)


def rj_energy_levels(ea, eb, ej, nvars, biases=None):
    """(kE, jhi, jlo per input edge, hhi, hlo per site): the two integer levels of that path's energies."""
    ea, eb, ej, b = _arr(ea, np.uint64), _arr(eb, np.uint64), _arr(ej, np.float64), _arr(biases, np.float64)
    jhi, jlo = np.zeros(len(ea), dtype=np.int32), np.zeros(len(ea), dtype=np.int32)
    hhi, hlo, k = np.zeros(nvars, dtype=np.int32), np.zeros(nvars, dtype=np.int32), C.c_int()
    _check(lib().isingmc_host_rj_energy_levels(_p(ea), _p(eb), _p(ej), len(ea), nvars, _p(b), _p(jhi), _p(jlo), _p(hhi), _p(hlo), C.byref(k)))
    return k.value, jhi, jlo, hhi, hlo


def rj_beta(beta, k):
    sh, mant = C.c_uint32(), C.c_uint32()
    _check(lib().isingmc_host_rj_beta(float(beta), int(k), C.byref(sh), C.byref(mant)))
    return sh.value, mant.value


def rj_log_table():
    out = np.zeros(2049, dtype=np.uint32)
    _check(lib().isingmc_host_rj_log_table(_p(out)))
    return out


def colour_graph(ea, eb, nvars):
    ea, eb = _arr(ea, np.uint64), _arr(eb, np.uint64)
    colours = np.zeros(nvars, dtype=np.uint32)
    nc = C.c_uint32()
    _check(lib().isingmc_host_colour_graph(_p(ea), _p(eb), len(ea), nvars, _p(colours), C.byref(nc)))
    return nc.value, colours


def pt_swap_round(seed, rnd, betas, slot_energy, perm):
    """One exchange round of the beta ladder; perm (uint32, rung -> slot) is updated in place."""
    betas, slot_energy = _arr(betas, np.float64), _arr(slot_energy, np.float64)
    assert perm.dtype == np.uint32 and perm.flags.c_contiguous
    swaps = C.c_uint64()
    _check(lib().isingmc_host_pt_swap_round(C.c_uint64(int(seed)), C.c_uint64(int(rnd)), len(betas), _p(betas),
                                            _p(slot_energy), _p(perm), C.byref(swaps)))
    return swaps.value


def pt_statistics_zeros(n_rungs):
    """The raw ladder statistics of a ladder of n_rungs before its first round: what States.pt_statistics()
    returns, as caller-held arrays for pt_statistics_round."""
    n = int(n_rungs)
    out = {k: np.zeros(max(n - 1, 0), dtype=np.uint64) for k in ("attempts", "accepts")}
    out.update({k: np.zeros(n, dtype=np.uint64) for k in ("n_up", "n_down", "round_trips")})
    out.update({k: np.zeros(n, dtype=np.float64) for k in ("sum_e", "sum_e2")})
    out["labels"] = np.zeros(n, dtype=np.uint8)
    out["rounds"], out["in_kernel_rounds"] = 0, 0
    return out


def pt_statistics_round(stats, rnd, perm_before, perm_after, slot_energy):
    """One exchange round's update of `stats` (pt_statistics_zeros) in place, after pt_swap_round: the host twin of the kernels."""
    pb, pa, e = _arr(perm_before, np.uint32), _arr(perm_after, np.uint32), _arr(slot_energy, np.float64)
    n = len(stats["labels"])
    if not (len(pb) == len(pa) == n and len(e) >= n):
        raise ValueError("permutations and energies must cover the ladder's rungs")
    for k, dt in (("attempts", np.uint64), ("accepts", np.uint64), ("n_up", np.uint64), ("n_down", np.uint64), ("sum_e", np.float64),
                  ("sum_e2", np.float64), ("round_trips", np.uint64), ("labels", np.uint8)):
        assert stats[k].dtype == dt and stats[k].flags.c_contiguous
    rounds = C.c_uint64(int(stats["rounds"]))
    _check(lib().isingmc_host_pt_statistics_round(C.c_uint64(int(rnd)), n, _p(pb), _p(pa), _p(e), _p(stats["attempts"]),
                                                  _p(stats["accepts"]), _p(stats["n_up"]), _p(stats["n_down"]), _p(stats["sum_e"]),
                                                  _p(stats["sum_e2"]), _p(stats["round_trips"]), _p(stats["labels"]), C.byref(rounds)))
    stats["rounds"] = rounds.value


def pa_sources(seed, step, energies, dbeta):
    """(src uint32[n], S, E_ref): the source table of one population-annealing resampling."""
    e = _arr(energies, np.float64)
    src = np.zeros(len(e), dtype=np.uint32)
    total, eref = C.c_uint64(), C.c_double()
    _check(lib().isingmc_host_pa_sources(C.c_uint64(int(seed)), C.c_uint64(int(step)), len(e), _p(e), float(dbeta), _p(src),
                                         C.byref(total), C.byref(eref)))
    return src, total.value, eref.value


def _pa_choice(call):
    """dict(k, dbeta, sum, num): the outputs of one of the two step choosers (num = N as a Python integer)."""
    k, dbeta, total, lo, hi = C.c_uint32(), C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(call(C.byref(k), C.byref(dbeta), C.byref(total), C.byref(lo), C.byref(hi)))
    return dict(k=k.value, dbeta=dbeta.value, sum=total.value, num=(hi.value << 64) | lo.value)


def pa_choose_step(energies, dbeta_max, target):
    """The temperature step of a population-annealing schedule from the energies, on the host."""
    e = _arr(energies, np.float64)
    return _pa_choice(lambda *out: lib().isingmc_host_pa_choose_step(len(e), _p(e), float(dbeta_max), float(target), *out))


NO_CLASS = 0xFFFFFFFF


def class_tables(tables, nvars, n_classes=None):
    """(uint32[n_tables, nvars], n_classes) of one table or a stack of them; n_classes defaults to the largest class + 1, NO_CLASS
    entries left aside."""
    t = np.atleast_2d(_arr(tables, np.uint32))
    if t.ndim != 2 or t.shape[1] != nvars:
        raise ValueError("class tables must be one array of nvars entries, or a stack [n_tables, nvars] of them")
    if n_classes is None:
        classed = t[t != NO_CLASS]
        n_classes = int(classed.max()) + 1 if classed.size else 1
    return np.ascontiguousarray(t), int(n_classes)


def class_segments(site, tables, n_classes):
    """(order, seg[n_seg, 4] = {table, class, first, count}, sizes[n_tables, n_classes]): the position lists of a class set on the
    replica-packed families from a position -> site table (0xFFFFFFFF on padding).  No device."""
    site = _arr(site, np.uint32)
    t = np.atleast_2d(_arr(tables, np.uint32))
    n_tables, nvars = t.shape
    order = np.zeros(max(n_tables * len(site), 1), dtype=np.uint32)
    seg = np.zeros((max(n_tables * (max(int(n_classes), 0) + len(site) // 1024), 1), 4), dtype=np.uint32)
    sizes = np.zeros((n_tables, max(int(n_classes), 0)), dtype=np.uint64)
    n_order, n_seg = C.c_size_t(), C.c_size_t()
    _check(lib().isingmc_host_class_segments(_p(site), len(site), _p(t), nvars, n_tables, int(n_classes), _p(order), C.byref(n_order),
                                             _p(seg), C.byref(n_seg), _p(sizes)))
    return order[:n_order.value], seg[:n_seg.value], sizes


class PtGroup:
    """isingmc_pt_group: the shards of one ladder (States objects with the ladder attached, one per device) driven from this
    thread; the energies travel by RCCL (dlopen'd inside the library) or by device copies.  backend: 0 auto, 1 RCCL, 2 copies."""

    def __init__(self, shards, backend=0):
        self.shards = list(shards)  # keeps them alive
        self._h = _vp()
        arr = (_vp * len(self.shards))(*[s._h for s in self.shards])
        _check(lib().isingmc_pt_group_create(arr, len(self.shards), backend, C.byref(self._h)))
        for s in self.shards:  # a shard that is closed (or finalised by the cycle collector, in any order) closes its groups first
            s._groups.append(self)

    @property
    def backend(self):
        return {1: "rccl", 2: "copy"}[lib().isingmc_pt_group_backend(self._h)]

    def allgather(self):
        _check(lib().isingmc_pt_group_allgather(self._h))

    def run(self, timesteps, swap_every):
        _check(lib().isingmc_pt_group_run(self._h, timesteps, swap_every))

    def synchronize(self):
        _check(lib().isingmc_pt_group_synchronize(self._h))

    def close(self):
        if self._h:
            lib().isingmc_pt_group_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def release_cached_resources():
    """Hand the library's idle device blocks, pinned host blocks, streams and events back to the runtime; bytes released."""
    return int(lib().isingmc_release_cached_resources())


def debug_live_blocks():
    """(device blocks, pinned host blocks) that owners inside the library hold right now (the caches' idle blocks not counted)."""
    dev, pinned = C.c_size_t(), C.c_size_t()
    _check(lib().isingmc_debug_live_blocks(C.byref(dev), C.byref(pinned)))
    return dev.value, pinned.value


class Graph:
    """isingmc_graph: edges (+ biases) resident on one device."""

    def __init__(self, ea, eb, ej, nvars=None, biases=None, device=0, force_general=False, stable_path=False):
        self._h = _vp()
        ea, eb, ej = _arr(ea, np.uint64), _arr(eb, np.uint64), _arr(ej, np.float64)
        if nvars is None:
            nvars = int(max(ea.max(), eb.max())) + 1 if len(ea) else 0
        biases = _arr(biases, np.float64)
        _check(lib().isingmc_graph_create(_p(ea), _p(eb), _p(ej), len(ea), nvars, _p(biases), device,
                                          (FLAG_FORCE_GENERAL if force_general else 0) | (FLAG_STABLE_PATH if stable_path else 0),
                                          C.byref(self._h)))
        self._children = []
        info = GraphInfo()
        _check(lib().isingmc_graph_info(self._h, C.byref(info)))
        self.info = info
        self.nvars = int(info.nvars)
        self.n_edges = int(info.n_edges)
        self.kind = int(info.kind)
        self.state_words = int(info.state_words)

    def family_for(self, n_experiments):
        """The kernel family a container of n_experiments created now on this graph would run on (FAMILIES)."""
        f = C.c_int()
        _check(lib().isingmc_graph_family_for(self._h, n_experiments, C.byref(f)))
        return FAMILIES[f.value]

    def close(self):
        if self._h:
            for ref in getattr(self, "_children", []):  # replica containers hold a pointer to the graph: they go first, whatever
                child = ref()                           # order the garbage collector finalises a reference cycle in
                if child is not None:
                    child.close()
            lib().isingmc_graph_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SiteClasses:
    """isingmc_site_classes: class tables over one graph, rearranged once for the kernels and kept on its device.
    tables: one table of nvars classes or a stack [n_tables, nvars], in the site numbering of the edge list; NO_CLASS = counted
    nowhere.  .sizes: uint64[n_tables, n_classes], the sites of every class."""

    def __init__(self, graph, tables, n_classes=None):
        self.graph = graph  # keeps the graph alive
        self._h = _vp()
        t, n_classes = class_tables(tables, graph.nvars, n_classes)
        self.n_tables, self.n_classes = t.shape[0], n_classes
        _check(lib().isingmc_site_classes_create(graph._h, _p(t), self.n_tables, n_classes, C.byref(self._h)))
        graph._children.append(weakref.ref(self))
        self.sizes = np.zeros((self.n_tables, n_classes), dtype=np.uint64)
        _check(lib().isingmc_site_classes_sizes(self._h, _p(self.sizes)))

    def close(self):
        if self._h:
            _close_series(self)
            lib().isingmc_site_classes_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SeriesHandle:
    """The handle of an overlap or observable series, shared by the series object and by everything it reads (its containers, its
    class set): whichever of them goes first destroys the series.  (Not a weak reference to the series object: the garbage collector
    clears those before it finalises a cycle, and the series must go before what it reads in whatever order that happens.)"""

    def __init__(self, destroy):
        self.h, self.destroy = _vp(), destroy

    def close(self):
        if self.h:
            getattr(lib(), self.destroy)(self.h)
            self.h = _vp()


def _close_series(owner):
    """The overlap and observable series that read `owner` (a container or a class set) go before it does."""
    for handle in owner.__dict__.pop("_series", []):
        handle.close()


class _DeviceSeries:
    """What the two device-resident logs share: the handle and its registration with the objects the series reads, the period, the
    row count and the capacity.  _PREFIX names the entry points of the subclass."""

    def _create(self, owners, *args):
        """isingmc_<kind>_series_create(*args, &handle); the owners given (None: absent) destroy the series when they go first."""
        self._handle = _SeriesHandle(self._PREFIX + "destroy")
        _check(self._call("create", *args, C.byref(self._handle.h)))
        for owner in owners:
            if owner is not None:
                owner.__dict__["_series"] = [h for h in owner.__dict__.get("_series", []) if h.h] + [self._handle]

    def _call(self, name, *args):
        return getattr(lib(), self._PREFIX + name)(*args)

    @property
    def _h(self):
        return self._handle.h

    def set_every(self, k):
        """A record follows every timestep t > t0 (now) with (t - t0) % k == 0, inside the run calls; 0: off, the rows stay."""
        _check(self._call("set_every", self._h, int(k)))

    @property
    def count(self):
        n = C.c_size_t()
        _check(self._call("count", self._h, C.byref(n), None))
        return int(n.value)

    @property
    def capacity(self):
        n = C.c_size_t()
        _check(self._call("count", self._h, None, C.byref(n)))
        return int(n.value)

    def _rows(self, first, n):
        first = int(first)
        return first, max(self.count - first, 0) if n is None else int(n)

    def reset(self):
        """The row count back to 0 (enqueue only); the period stays."""
        _check(self._call("reset", self._h))

    def close(self):
        self._handle.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OverlapSeries(_DeviceSeries):
    """isingmc_overlap_series: a device-resident log with one row of overlaps per sample.  record() and the
    periodic records inside the step loop only enqueue; get() reads the log, once, afterwards.  Made by States.overlap_series."""

    _PREFIX = "isingmc_overlap_series_"

    def __init__(self, a, other=None, n_pairs=None, classes=None, link=True, by_rung=False, capacity=4096):
        self._a, self._b, self._classes = a, other, classes  # keeps them alive
        if n_pairs is None:
            n_pairs = a.count if by_rung else a.count // 2 if other is None or other is a else min(a.count, other.count)
        self.n_pairs, self.link, self.by_rung = int(n_pairs), bool(link), bool(by_rung)
        self.n_tables, self.n_classes = (classes.n_tables, classes.n_classes) if classes is not None else (0, 0)
        flags = (SERIES_LINK if link else 0) | (SERIES_BY_RUNG if by_rung else 0)
        self._create((a, other, classes), a._h, None if other is None else other._h, self.n_pairs,
                     None if classes is None else classes._h, flags, int(capacity))

    def record(self, slots_a=None, slots_b=None):
        """One row for the configurations as they are; pairs as States.overlaps takes them.  Enqueue only."""
        if (slots_a is None) != (slots_b is None):
            raise ValueError("give both slot tables or neither")
        sa, sb = _arr(slots_a, np.uint32), _arr(slots_b, np.uint32)
        if sa is not None and (sa.ndim != 1 or sa.shape != sb.shape or sa.size != self.n_pairs):
            raise ValueError("the slot tables must be two one-dimensional arrays of n_pairs entries")
        _check(self._call("record", self._h, _p(sa), _p(sb)))

    def get(self, first=0, n=None):
        """(timesteps uint64[n], spin int64[n, P], link int64[n, P] or None, by_class int64[n, P, T, C] or None) of the rows
        [first, first + n) (n=None: all from `first` on).  Synchronises; changes nothing."""
        first, n = self._rows(first, n)
        P = self.n_pairs
        t = np.zeros(n, dtype=np.uint64)
        spin = np.zeros((n, P), dtype=np.int64)
        lnk = np.zeros((n, P), dtype=np.int64) if self.link else None
        cls = np.zeros((n, P, self.n_tables, self.n_classes), dtype=np.int64) if self.n_tables else None
        _check(self._call("get", self._h, first, n, _p(t), _p(spin), _p(lnk), _p(cls)))
        return t, spin, lnk, cls


class ObservableSeries(_DeviceSeries):
    """isingmc_observable_series: a device-resident log with one row per sample -- per column (replica slot, or rung with by_rung)
    the energy, the magnetisation and the magnetisation by site class.  record() and the periodic records inside
    the step loop only enqueue; get() reads the log, once, afterwards.  Made by States.observable_series."""

    _PREFIX = "isingmc_observable_series_"

    def __init__(self, a, classes=None, energy=True, magnetisation=True, by_rung=False, capacity=4096):
        self._a, self._classes = a, classes  # keeps them alive
        self.energy, self.magnetisation, self.by_rung = bool(energy), bool(magnetisation), bool(by_rung)
        self.n_columns = a.count
        self.n_tables, self.n_classes = (classes.n_tables, classes.n_classes) if classes is not None else (0, 0)
        flags = (OBS_ENERGY if energy else 0) | (OBS_MAGNETISATION if magnetisation else 0) | (OBS_BY_RUNG if by_rung else 0)
        self._create((a, classes), a._h, None if classes is None else classes._h, flags, int(capacity))

    def record(self):
        """One row for the configurations as they are.  Enqueue only."""
        _check(self._call("record", self._h))

    def get(self, first=0, n=None):
        """(timesteps uint64[n], energy float64[n, C] or None, magnetisation int64[n, C] or None, by_class int64[n, C, T, K] or
        None) of the rows [first, first + n) (n=None: all from `first` on).  Synchronises once; changes nothing."""
        first, n = self._rows(first, n)
        cols = self.n_columns
        t = np.zeros(n, dtype=np.uint64)
        e = np.zeros((n, cols), dtype=np.float64) if self.energy else None
        m = np.zeros((n, cols), dtype=np.int64) if self.magnetisation else None
        cls = np.zeros((n, cols, self.n_tables, self.n_classes), dtype=np.int64) if self.n_tables else None
        _check(self._call("get", self._h, first, n, _p(t), _p(e), _p(m), _p(cls)))
        return t, e, m, cls


CLUSTER_SERIES_KINDS = {"sw": 0, "icm": 1}  # ISINGMC_CLUSTER_SERIES_*


class ClusterSeries(_DeviceSeries):
    """isingmc_cluster_series: a device-resident log with one row per non-local step of its container -- per column (replica of a
    Swendsen-Wang step, pair of an isoenergetic cluster move) the number of clusters, the largest, and the sums of s, s^2 and s^4
    over the cluster sizes.  The steps append the rows themselves, enqueue only; get() reads the log, once,
    afterwards.  Made by States.cluster_series."""

    _PREFIX = "isingmc_cluster_series_"

    def __init__(self, a, kind="sw", capacity=4096):
        if kind not in CLUSTER_SERIES_KINDS:
            raise ValueError("kind must be 'sw' (Swendsen-Wang steps) or 'icm' (isoenergetic cluster moves)")
        self._a = a  # keeps it alive
        self.kind = kind
        self.n_columns = a.count if kind == "sw" else a.count // 2
        self._create((a,), a._h, CLUSTER_SERIES_KINDS[kind], int(capacity))

    def set_every(self, k):
        """A cluster series has no period of its own: its rows are the container's non-local steps (States.set_cluster_every /
        set_icm_every)."""
        raise TypeError("a cluster series has no period of its own: its rows follow set_cluster_every / set_icm_every of the container")

    def get(self, first=0, n=None):
        """(timesteps uint64[n], n_clusters, largest, sites, s2, s4_lo, s4_hi: uint64[n, C] each) of the rows [first, first + n)
        (n=None: all from `first` on); sum s^4 = s4_hi 2^64 + s4_lo.  Synchronises once; changes nothing."""
        first, n = self._rows(first, n)
        t = np.zeros(n, dtype=np.uint64)
        rows = np.zeros((n, self.n_columns, 6), dtype=np.uint64)
        _check(self._call("get", self._h, first, n, _p(t), _p(rows)))
        return (t,) + tuple(np.ascontiguousarray(rows[:, :, i]) for i in range(6))


def autocorr_plan(samples_taken, n_lags):
    """(slot_of_lag uint32[L + 1], live_lags, write_slot, counts uint64[L + 1]): the bookkeeping of a lag ring of L = n_lags snapshots
    when samples_taken samples are in it, as the launch of the next sample uses it.  No device."""
    L = int(n_lags)
    slots, counts = np.zeros(max(L, 0) + 1, dtype=np.uint32), np.zeros(max(L, 0) + 1, dtype=np.uint64)
    live, write = C.c_uint32(), C.c_uint32()
    _check(lib().isingmc_host_autocorr_plan(C.c_uint64(int(samples_taken)), L, _p(slots), C.byref(live), C.byref(write), _p(counts)))
    return slots, int(live.value), int(write.value), counts


class Autocorrelation:
    """isingmc_autocorr: the lag ring of a container -- L snapshots of its configurations on the device and, per
    replica and lag l = 1 .. L, the number of sites that differ between a sample and the sample l samples before it, summed over
    the samples.  sample() and the periodic samples inside the step loop only enqueue one launch; get() reads the sums, once,
    afterwards.  Made by States.autocorrelation; one ring per container."""

    def __init__(self, a, n_lags):
        self._a = a  # keeps it alive
        self._handle = _SeriesHandle("isingmc_autocorr_destroy")
        _check(lib().isingmc_autocorr_create(a._h, int(n_lags), 0, C.byref(self._handle.h)))
        a.__dict__["_series"] = [h for h in a.__dict__.get("_series", []) if h.h] + [self._handle]  # (the ring goes before its container)

    @property
    def _h(self):
        return self._handle.h

    def set_every(self, k):
        """A sample follows every timestep t > t0 (now) with (t - t0) % k == 0, whatever kind of timestep it is, inside the run
        calls; 0: off, ring and sums stay."""
        _check(lib().isingmc_autocorr_set_every(self._h, int(k)))

    def sample(self):
        """One sample of the configurations as they are.  Enqueue only."""
        _check(lib().isingmc_autocorr_sample(self._h))

    @property
    def samples(self):
        """Samples taken since creation or the last reset."""
        n = C.c_uint64()
        _check(lib().isingmc_autocorr_count(self._h, C.byref(n), None))
        return int(n.value)

    @property
    def n_lags(self):
        n = C.c_size_t()
        _check(lib().isingmc_autocorr_count(self._h, None, C.byref(n)))
        return int(n.value)

    def get(self):
        """(counts uint64[L + 1], diff uint64[R, L + 1]): the terms in every lag, max(0, samples - l), and per replica the sum over
        them of the sites that differ; diff[:, 0] is 0.  correlation.autocorrelation turns them into C.  Synchronises once; changes nothing."""
        L = self.n_lags
        counts, diff = np.zeros(L + 1, dtype=np.uint64), np.zeros((self._a.count, L + 1), dtype=np.uint64)
        _check(lib().isingmc_autocorr_get(self._h, _p(counts), _p(diff)))
        return counts, diff

    def reset(self):
        """Sums and sample number back to 0 (enqueue only); the period stays."""
        _check(lib().isingmc_autocorr_reset(self._h))

    def run_sampling(self, beta, thermalization, sampling_freq, n_samples, site_sums=False):
        """The loop of States.run_sampling with the samples taken by the ring (reset first) instead of copied out: the final
        energies float64[R], one wait.  site_sums: the per-replica site sums (States.moments) take the same samples."""
        energies = np.zeros(self._a.count, dtype=np.float64)
        _check(lib().isingmc_run_sampling_autocorr(self._h, float(0.0 if beta is None else beta), int(thermalization), int(sampling_freq),
                                                   int(n_samples), int(bool(site_sums)), _p(energies)))
        return energies

    def close(self):
        self._handle.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nonlocal_steps(t0, timesteps, k):
    """The timesteps t in [t0, t0 + timesteps) with t % k == k - 1 (0 when k == 0): the rows a run call appends to a cluster series."""
    out = C.c_uint64()
    _check(lib().isingmc_host_nonlocal_steps(C.c_uint64(int(t0)), int(timesteps), int(k), C.byref(out)))
    return int(out.value)


class States:
    """isingmc_states: R replicas of the graph's spins on the device."""

    def __init__(self, graph, seeds, initial_state=None, replica_range=None):
        """seeds: one u64 per experiment.  replica_range=(lo, hi): this object is the shard [lo, hi) of the
        len(seeds) experiments (isingmc_states_create_range: results do not depend on the cut)."""
        self.graph = graph  # keeps the graph alive
        self._groups = []
        self._h = _vp()
        seeds = _arr(seeds, np.uint64)
        ini = _arr(initial_state, np.uint8)
        if ini is not None and ini.size != graph.nvars:
            raise ValueError("Initial state must be of the same size as biases, or 0.")
        if replica_range is None:
            _check(lib().isingmc_states_create(graph._h, len(seeds), _p(seeds), _p(ini), C.byref(self._h)))
        else:
            lo, hi = int(replica_range[0]), int(replica_range[1])
            if not 0 <= lo <= hi <= len(seeds):
                raise ValueError("replica_range out of bounds")
            _check(lib().isingmc_states_create_range(graph._h, len(seeds), _p(seeds), lo, hi - lo, _p(ini),
                                                     C.byref(self._h)))
        graph._children.append(weakref.ref(self))

    @property
    def count(self):
        return int(lib().isingmc_states_count(self._h))

    @property
    def timestep(self):
        return int(lib().isingmc_states_timestep(self._h))

    @timestep.setter
    def timestep(self, t):
        _check(lib().isingmc_states_set_timestep(self._h, C.c_uint64(int(t))))

    def append(self, seed, initial_state=None):
        ini = _arr(initial_state, np.uint8)
        _check(lib().isingmc_states_append(self._h, C.c_uint64(int(seed)), _p(ini)))

    def set_state(self, replica, state):
        st = _arr(state, np.uint8)
        if st.size != self.graph.nvars:
            raise ValueError("Initial state must be of the same size as biases, or 0.")
        _check(lib().isingmc_states_set_state(self._h, replica, _p(st)))

    @property
    def family(self):
        """'checkerboard', 'csr_f64', 'packed_bitsliced' or 'packed_real': the kernel family this container runs on."""
        f = C.c_int()
        _check(lib().isingmc_states_family(self._h, C.byref(f)))
        return FAMILIES[f.value]

    def set_option(self, name, value):
        """One of the path / tuning switches of this container (the ISINGMC_* variable's name without the prefix)."""
        _check(lib().isingmc_states_set_option(self._h, name.encode(), int(value)))

    @property
    def philox_rounds(self):
        """Rounds of Philox4x32 in the draws of this container's sweeps: 10, or 7 after set_option("philox_rounds", 7) /
        ISINGMC_PHILOX_ROUNDS=7 on a periodic, field-free, one-|J| checkerboard lattice."""
        r = C.c_int()
        _check(lib().isingmc_states_philox_rounds(self._h, C.byref(r)))
        return r.value

    def set_betas(self, betas):
        b = _arr(betas, np.float64)
        if b is not None and b.size != self.count:
            raise ValueError("one beta per replica expected")
        _check(lib().isingmc_states_set_betas(self._h, _p(b)))

    def set_cluster_every(self, k):
        """Every k-th timestep (t % k == k - 1) becomes a Swendsen-Wang cluster step; 0 switches it off."""
        _check(lib().isingmc_states_set_cluster_every(self._h, int(k)))

    @property
    def cluster_every(self):
        k = C.c_size_t()
        _check(lib().isingmc_states_cluster_every(self._h, C.byref(k)))
        return int(k.value)

    def cluster_stats(self):
        """(number of clusters, size of the largest cluster) of every replica's last cluster step: two uint64[R] arrays."""
        n, largest = np.zeros(self.count, dtype=np.uint64), np.zeros(self.count, dtype=np.uint64)
        _check(lib().isingmc_cluster_stats(self._h, _p(n), _p(largest)))
        return n, largest

    def set_icm_every(self, k):
        """Every k-th timestep (t % k == k - 1) becomes an isoenergetic cluster move between the replicas (2p, 2p + 1)
        (DESIGN.md S9); 0 switches it off."""
        _check(lib().isingmc_states_set_icm_every(self._h, int(k)))

    @property
    def icm_every(self):
        k = C.c_size_t()
        _check(lib().isingmc_states_icm_every(self._h, C.byref(k)))
        return int(k.value)

    def icm_stats(self):
        """(number of q = -1 clusters, size of the largest, number of q = -1 sites) of every pair's last isoenergetic cluster
        move: three uint64[count // 2] arrays."""
        out = [np.zeros(self.count // 2, dtype=np.uint64) for _ in range(3)]
        _check(lib().isingmc_icm_stats(self._h, _p(out[0]), _p(out[1]), _p(out[2])))
        return tuple(out)

    def icm_between(self, other, slots_a=None, slots_b=None):
        """One isoenergetic cluster move between this container and `other` as timestep t of both: pair p =
        (replica slots_a[p] of self, replica slots_b[p] of other).  Without tables both containers carry a tempering ladder over
        the same betas and pair r = the two replicas at rung r (read on the device).  Enqueue only."""
        if (slots_a is None) != (slots_b is None):
            raise ValueError("give both slot tables or neither")
        if slots_a is None:
            sa, sb, n = None, None, self.count
        else:
            sa, sb = _arr(slots_a, np.uint32), _arr(slots_b, np.uint32)
            if sa.ndim != 1 or sa.shape != sb.shape:
                raise ValueError("the slot tables must be two one-dimensional arrays of one length")
            n = sa.size
        _check(lib().isingmc_icm_between(self._h, other._h, _p(sa), _p(sb), n))
        self._icmb_pairs = n

    def icm_between_stats(self):
        """(number of q = -1 clusters, size of the largest, number of q = -1 sites) per pair of the last icm_between call made
        on this container: three uint64[n_pairs] arrays."""
        n = getattr(self, "_icmb_pairs", 0)
        out = [np.zeros(n, dtype=np.uint64) for _ in range(3)]
        _check(lib().isingmc_icm_between_stats(self._h, _p(out[0]), _p(out[1]), _p(out[2]), n))
        return tuple(out)

    def _overlap_pairs(self, other, slots_a, slots_b):
        """(slots_a, slots_b, n_pairs) as isingmc_overlaps and isingmc_overlaps_by_class take them."""
        if (slots_a is None) != (slots_b is None):
            raise ValueError("give both slot tables or neither")
        if slots_a is None:
            sa, sb = None, None
            n = self.count // 2 if other is None or other is self else min(self.count, other.count)
        else:
            sa, sb = _arr(slots_a, np.uint32), _arr(slots_b, np.uint32)
            if sa.ndim != 1 or sa.shape != sb.shape:
                raise ValueError("the slot tables must be two one-dimensional arrays of one length")
            n = sa.size
        return sa, sb, n

    def overlaps(self, other=None, slots_a=None, slots_b=None, link=True):
        """(spin, link): int64[n_pairs] each, spin[p] = sum_i s_i s'_i and link[p] = sum over the edge-list entries of
        s_a s_b s'_a s'_b for pair p; link is None when not asked for.  Without tables: the pairs (2p, 2p + 1) of
        this container, or with `other` pair p = (slot p of self, slot p of other) up to the smaller count; with tables pair p =
        (slot slots_a[p] of self, slot slots_b[p] of `other`, or of self without one).  Reads only; synchronises."""
        sa, sb, n = self._overlap_pairs(other, slots_a, slots_b)
        spin = np.zeros(n, dtype=np.int64)
        lnk = np.zeros(n, dtype=np.int64) if link else None
        _check(lib().isingmc_overlaps(self._h, None if other is None else other._h, _p(sa), _p(sb), n, _p(spin), _p(lnk)))
        return spin, lnk

    def overlaps_by_class(self, classes, other=None, slots_a=None, slots_b=None):
        """int64[n_pairs, n_tables, n_classes]: out[p, t, c] = the sum of s_i s'_i over the sites i of class c of table t
        (DESIGN.md S17), for the pairs overlaps() would take with the same arguments.  classes: a SiteClasses of this graph.
        Reads only; synchronises."""
        sa, sb, n = self._overlap_pairs(other, slots_a, slots_b)
        out = np.zeros((n, classes.n_tables, classes.n_classes), dtype=np.int64)
        _check(lib().isingmc_overlaps_by_class(self._h, None if other is None else other._h, _p(sa), _p(sb), n, classes._h, _p(out)))
        return out

    def observable_series(self, classes=None, energy=True, magnetisation=True, by_rung=False, capacity=4096):
        """An ObservableSeries: energy, magnetisation and magnetisation by class of every replica (by_rung: of
        every rung of the attached ladder), one row per record, kept on the device."""
        return ObservableSeries(self, classes, energy, magnetisation, by_rung, capacity)

    def cluster_series(self, kind="sw", capacity=4096):
        """A ClusterSeries: the cluster-size moments of every Swendsen-Wang step (kind="sw", a column per replica)
        or isoenergetic cluster move (kind="icm", a column per pair (2p, 2p + 1)) of this container, one row per step, kept on the
        device.  One live cluster series per container."""
        return ClusterSeries(self, kind, capacity)

    def overlap_series(self, other=None, n_pairs=None, classes=None, link=True, by_rung=False, capacity=4096):
        """An OverlapSeries over the pairs overlaps() would take: one row per record, kept on the device.
        n_pairs=None: count // 2 inside this container, the smaller count between two, the number of rungs with by_rung (both
        containers carry a whole ladder over equal betas; pair r = the two replicas at rung r, read on the device)."""
        return OverlapSeries(self, other, n_pairs, classes, link, by_rung, capacity)

    def autocorrelation(self, n_lags):
        """An Autocorrelation: the lag ring of this container, n_lags = 1 .. 256 snapshots kept on the device.  One
        ring per container; ValueError where isingmc_autocorr_create refuses."""
        return Autocorrelation(self, n_lags)

    # ---- each replica's lowest-energy configuration
    def set_track_best(self, k):
        """An update of the records follows every timestep after which t % k == 0; 0 switches tracking off."""
        _check(lib().isingmc_states_set_track_best(self._h, int(k)))

    @property
    def track_best(self):
        k = C.c_size_t()
        _check(lib().isingmc_states_track_best(self._h, C.byref(k)))
        return int(k.value)

    def best_update(self):
        """One update at the current timestep, whatever the period; enqueue only."""
        _check(lib().isingmc_best_update(self._h))

    def best(self, states=True):
        """(energies float64[R], states bool[R, nvars] or None, timesteps uint64[R], improvements): every replica's record, the
        configuration it was set with and the timestep of that update; how often a record has been set.  Synchronises."""
        R, N = self.count, self.graph.nvars
        e, t = np.zeros(R, dtype=np.float64), np.zeros(R, dtype=np.uint64)
        st = np.zeros((R, N), dtype=np.bool_) if states else None
        n = C.c_uint64()
        _check(lib().isingmc_best_get(self._h, _p(e), None if st is None else st.ctypes.data_as(_vp), N, _p(t), C.byref(n)))
        return e, st, t, int(n.value)

    def best_raw(self):
        """The second state buffer's words as they lie in memory, uint32 (one-dimensional), as raw_state()."""
        n = C.c_size_t()
        _check(lib().isingmc_best_raw_state(self._h, None, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        _check(lib().isingmc_best_raw_state(self._h, _p(out), None))
        return out

    def best_reset(self):
        _check(lib().isingmc_best_reset(self._h))

    # ---- per-site spin sums and per-bond sums over the samples of a run
    def set_moments_every(self, every, per_replica=False, bonds=False, per_rung=False):
        """A sample of all replicas follows every timestep t > t0 (now) with (t - t0) % every == 0; 0 switches accumulation off and
        keeps the sums.  per_replica: sums per replica instead of over all of them; bonds: the sums of s_a s_b per edge-list entry too.
        per_rung: a container with a whole tempering ladder attached -- sums per rung, whichever slot holds it."""
        flags = (MOMENTS_PER_REPLICA if per_replica else 0) | (MOMENTS_BONDS if bonds else 0) | (MOMENTS_PER_RUNG if per_rung else 0)
        _check(lib().isingmc_states_set_moments_every(self._h, int(every), flags))

    @property
    def moments_every(self):
        """(every, per_replica, bonds) as set."""
        k, f = C.c_size_t(), C.c_uint()
        _check(lib().isingmc_states_moments_every(self._h, C.byref(k), C.byref(f)))
        return int(k.value), bool(f.value & MOMENTS_PER_REPLICA), bool(f.value & MOMENTS_BONDS)

    @property
    def moments_per_rung(self):
        """Are the sums held (or last set) the sums per rung of a tempering ladder?"""
        f = C.c_uint()
        _check(lib().isingmc_states_moments_every(self._h, None, C.byref(f)))
        return bool(f.value & MOMENTS_PER_RUNG)

    def accumulate_moments(self):
        """One sample at the current timestep, whatever the period; enqueue only."""
        _check(lib().isingmc_moments_accumulate(self._h))

    def moments(self):
        """(n, site, bond or None): the samples taken and the exact integer sums, True = +1 -- site int64[nvars] (int64[R, nvars] per
        replica, int64[n_rungs, nvars] in ladder order per rung), bond int64[n_edges] in the order of the edge list when bond sums are
        held.  Synchronises."""
        _, per_replica, bonds = self.moments_every
        N = self.graph.nvars
        site = np.zeros((self.count, N) if per_replica or self.moments_per_rung else N, dtype=np.int64)
        bond = np.zeros(self.graph.n_edges, dtype=np.int64) if bonds else None
        n = C.c_uint64()
        _check(lib().isingmc_moments_get(self._h, C.byref(n), _p(site), _p(bond)))
        return int(n.value), site, bond

    def reset_moments(self):
        _check(lib().isingmc_moments_reset(self._h))

    def run_sampling_moments(self, beta, thermalization, sampling_freq, n_samples, per_replica=False, bonds=False):
        """The loop of run_sampling with the samples summed on the device: the final energies float64[R]; moments() reads the sums."""
        flags = (MOMENTS_PER_REPLICA if per_replica else 0) | (MOMENTS_BONDS if bonds else 0)
        energies = np.zeros(self.count, dtype=np.float64)
        _check(lib().isingmc_run_sampling_moments(self._h, float(0.0 if beta is None else beta), thermalization, sampling_freq, n_samples,
                                                  flags, _p(energies)))
        return energies

    def do_time_steps(self, timesteps, beta=None, per_step_energies=False):
        """beta: float (constant), sequence of length timesteps, or None when per-replica betas are set."""
        R = self.count
        if beta is None:
            b, stride = None, 0
        elif np.ndim(beta) == 0:
            b, stride = np.array([beta], dtype=np.float64), 0
        else:
            b, stride = _arr(beta, np.float64), 1
            if b.size != timesteps:
                raise ValueError("need one beta per timestep")
        out = np.zeros((R, timesteps), dtype=np.float64) if per_step_energies else None
        _check(lib().isingmc_do_time_steps(self._h, timesteps, _p(b), stride, _p(out)))
        return out

    def do_time_steps_timed(self, timesteps, beta):
        b = np.array([beta], dtype=np.float64) if np.ndim(beta) == 0 else _arr(beta, np.float64)
        ms = C.c_float()
        _check(lib().isingmc_do_time_steps_timed(self._h, timesteps, _p(b), 0 if b.size == 1 else 1, C.byref(ms)))
        return ms.value

    def run_sampling(self, beta, thermalization, sampling_freq, n_samples):
        """(energies float64[R, S], states bool[R, S, nvars]) -- the sampling loop of lattice.rs:271-287."""
        R, N = self.count, self.graph.nvars
        energies = np.zeros((R, n_samples), dtype=np.float64)
        states = np.zeros((R, n_samples, N), dtype=np.bool_)
        _check(lib().isingmc_run_sampling(self._h, float(0.0 if beta is None else beta), thermalization, sampling_freq,
                                          n_samples, _p(energies), states.ctypes.data_as(_vp)))
        return energies, states

    def energies(self):
        out = np.zeros(self.count, dtype=np.float64)
        _check(lib().isingmc_get_energies(self._h, _p(out)))
        return out

    def magnetisations(self):
        out = np.zeros(self.count, dtype=np.int64)
        _check(lib().isingmc_get_magnetisations(self._h, _p(out)))
        return out

    def states(self, out=None):
        """bool[R, nvars]; `out` may be a C-contiguous (R, ..., nvars)-strided uint8/bool view base."""
        R, N = self.count, self.graph.nvars
        if out is None:
            out = np.zeros((R, N), dtype=np.bool_)
            stride = N
        else:
            stride = out.strides[0]
        _check(lib().isingmc_get_states(self._h, out.ctypes.data_as(_vp), stride))
        return out

    def packed(self):
        out = np.zeros((self.count, self.graph.state_words), dtype=np.uint32)
        _check(lib().isingmc_get_packed_states(self._h, _p(out)))
        return out

    # ---- on-stream parallel tempering (lattice path): every call below only ENQUEUES on the engine's stream
    def pt_attach(self, ladder_betas, slot_offset, slots_per_rank, world_size, seed):
        b = _arr(ladder_betas, np.float64)
        _check(lib().isingmc_pt_attach(self._h, _p(b), len(b), slot_offset, slots_per_rank, world_size,
                                       C.c_uint64(int(seed))))
        self._pt_rungs = len(b)
        self._pt_world = world_size

    def pt_can_attach(self, n_rungs, slot_offset, slots_per_rank, world_size):
        """Would pt_attach accept this container and ladder geometry?  No side effects."""
        ok = C.c_int()
        _check(lib().isingmc_pt_can_attach(self._h, n_rungs, slot_offset, slots_per_rank, world_size, C.byref(ok)))
        return bool(ok.value)

    def pt_detach(self):
        _check(lib().isingmc_pt_detach(self._h))

    def pt_buffers(self):
        """(local, all) as torch CUDA tensors viewing the engine's device buffers (no copy)."""
        import torch
        loc, al, per = _vp(), _vp(), C.c_size_t()
        _check(lib().isingmc_pt_buffers(self._h, C.byref(loc), C.byref(al), C.byref(per)))

        class _View:  # __cuda_array_interface__ view of a raw device pointer
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        dev = torch.device("cuda", self.graph.info.device)
        world = self._pt_world
        return (torch.as_tensor(_View(loc.value, per.value), device=dev),
                torch.as_tensor(_View(al.value, per.value * world), device=dev))

    def pt_stream(self):
        import torch
        st = _vp()
        _check(lib().isingmc_states_stream(self._h, C.byref(st)))
        return torch.cuda.ExternalStream(st.value, device=torch.device("cuda", self.graph.info.device))

    def pt_time_steps(self, timesteps):
        _check(lib().isingmc_pt_time_steps(self._h, timesteps))

    def pt_run(self, timesteps, swap_every):
        _check(lib().isingmc_pt_run(self._h, timesteps, swap_every))

    def pt_measure(self):
        _check(lib().isingmc_pt_measure(self._h))

    def pt_swap(self):
        _check(lib().isingmc_pt_swap(self._h))

    def pt_state(self):
        perm = np.zeros(self._pt_rungs, dtype=np.uint32)
        rnd, swaps = C.c_uint64(), C.c_uint64()
        _check(lib().isingmc_pt_state(self._h, _p(perm), C.byref(rnd), C.byref(swaps)))
        return perm, rnd.value, swaps.value

    # ---- ladder statistics
    def pt_set_statistics(self, on=True):
        _check(lib().isingmc_pt_set_statistics(self._h, int(bool(on))))

    def pt_statistics(self):
        """The raw statistics (synchronises): dict(rounds, in_kernel_rounds, attempts, accepts, n_up, n_down, sum_e, sum_e2 by rung /
        pair, round_trips, labels by global slot)."""
        out = pt_statistics_zeros(getattr(self, "_pt_rungs", 0))
        rounds, inside = C.c_uint64(), C.c_uint64()
        _check(lib().isingmc_pt_statistics_get(self._h, C.byref(rounds), C.byref(inside), *(_p(out[k]) for k in (
            "attempts", "accepts", "n_up", "n_down", "sum_e", "sum_e2", "round_trips", "labels"))))
        out["rounds"], out["in_kernel_rounds"] = rounds.value, inside.value
        return out

    def pt_reset_statistics(self):
        _check(lib().isingmc_pt_statistics_reset(self._h))

    def raw_state(self):
        """The device words as they lie in memory, uint32 (one-dimensional): padding and unowned bits of a packed container included."""
        n = C.c_size_t()
        _check(lib().isingmc_get_raw_state(self._h, None, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        _check(lib().isingmc_get_raw_state(self._h, _p(out), None))
        return out

    # ---- population annealing
    def pa_run(self, betas, sweeps_per_beta, seed):
        """The whole schedule with one host wait at the end: dict(sum, eref, distinct, mean_energy), one entry per resampling."""
        b = _arr(betas, np.float64)
        n = max(len(b) - 1, 0)
        total, distinct = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        eref, mean = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        _check(lib().isingmc_pa_run(self._h, _p(b), len(b), int(sweeps_per_beta), C.c_uint64(int(seed)), _p(total), _p(eref), _p(distinct), _p(mean)))
        return dict(sum=total, eref=eref, distinct=distinct, mean_energy=mean)

    def pa_choose_step(self, dbeta_max, target):
        """dict(k, dbeta, sum, num) of the step chosen for the population as it stands; reads only, synchronises."""
        return _pa_choice(lambda *out: lib().isingmc_pa_choose_step(self._h, float(dbeta_max), float(target), *out))

    def pa_run_adaptive(self, beta_start, beta_end, sweeps_per_beta, seed, target, dbeta_cap=None, max_steps=10000):
        """A schedule whose steps are chosen as it runs: dict(betas, sum, eref, distinct, mean_energy), one record per step.  A
        ValueError for a max_steps that does not reach beta_end carries what was completed as its attribute `partial`."""
        betas, n = np.zeros(max_steps + 1, dtype=np.float64), C.c_size_t()
        total, distinct = np.zeros(max_steps, dtype=np.uint64), np.zeros(max_steps, dtype=np.uint64)
        eref, mean = np.zeros(max_steps, dtype=np.float64), np.zeros(max_steps, dtype=np.float64)
        cap = float("inf") if dbeta_cap is None else float(dbeta_cap)
        rc = lib().isingmc_pa_run_adaptive(self._h, float(beta_start), float(beta_end), int(sweeps_per_beta), C.c_uint64(int(seed)), float(target),
                                           cap, int(max_steps), _p(betas), C.byref(n), _p(total), _p(eref), _p(distinct), _p(mean))
        m = max(n.value, 1) - 1
        out = dict(betas=betas[:n.value].copy(), sum=total[:m].copy(), eref=eref[:m].copy(), distinct=distinct[:m].copy(), mean_energy=mean[:m].copy())
        try:
            _check(rc)
        except ValueError as e:
            e.partial = out
            raise
        return out

    def pa_resample(self, dbeta, seed, step):
        """Resample the population for the step dbeta = beta_to - beta_from; enqueue only."""
        _check(lib().isingmc_pa_resample(self._h, float(dbeta), C.c_uint64(int(seed)), C.c_uint64(int(step))))

    def pa_apply_sources(self, src):
        """new slot j <- old replica src[j] for any table with entries below the replica count."""
        t = _arr(src, np.uint32)
        if t.ndim != 1 or t.size != self.count:
            raise ValueError("one source per replica expected")
        _check(lib().isingmc_pa_apply_sources(self._h, _p(t)))

    def pa_last(self):
        """dict(src, sum, eref, distinct, mean_energy) of the last pa_resample (synchronises)."""
        src = np.zeros(self.count, dtype=np.uint32)
        total, eref, distinct, mean = C.c_uint64(), C.c_double(), C.c_uint64(), C.c_double()
        _check(lib().isingmc_pa_last(self._h, _p(src), C.byref(total), C.byref(eref), C.byref(distinct), C.byref(mean)))
        return dict(src=src, sum=total.value, eref=eref.value, distinct=distinct.value, mean_energy=mean.value)

    def pa_families(self):
        out = np.zeros(self.count, dtype=np.uint32)
        _check(lib().isingmc_pa_families(self._h, _p(out)))
        return out

    def pa_reset_families(self):
        _check(lib().isingmc_pa_reset_families(self._h))

    def synchronize(self):
        _check(lib().isingmc_synchronize(self._h))

    def shader_clock_ghz(self, timesteps, beta, probe_ms=10.0):
        """Shader clock held while `timesteps` sweeps run (measurement hook of bench.py)."""
        ghz = C.c_double()
        _check(lib().isingmc_debug_shader_clock(self._h, timesteps, float(beta), float(probe_ms), C.byref(ghz)))
        return ghz.value

    def close(self):
        if self._h:
            for grp in getattr(self, "_groups", []):
                grp.close()
            _close_series(self)
            lib().isingmc_states_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
