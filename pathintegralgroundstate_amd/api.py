"""Host-side mirror of the reference's procedure interface over the C ABI (include/pigs_hip.h).

The reference boundary is the Fortran call interface: ``UpdateAction``
(reference vpi_mod.f90:2491), ``PotentialEnergy`` / ``LocalEnergy`` / ``ThermEnergy``
(reference sample_mod.f90:13,154,323).  :class:`PigsContext` exposes the same operations with
the same argument meaning (ip 1-based, ib 0-based, arrays in the reference's column-major
layout, i.e. numpy C-order ``(M, Np, dim)`` for ``Path(dim,Np,0:2*Nb)``), batched over walkers.
All compute happens in ``libpigs_hip.so``; if that library or a GPU is missing every call
raises :class:`PigsError` -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .system import SystemConfig

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpigs_hip.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)

CL_NP_MAX = 2048           # PIGS_CL_NP_MAX of include/pigs_hip.h (pigs_cl_np_max() of the library)

# every symbol include/pigs_hip.h declares
ABI_SYMBOLS = [
    "pigs_ctx_create", "pigs_ctx_destroy", "pigs_last_error", "pigs_abi_version",
    "pigs_device_count", "pigs_sync", "pigs_stream", "pigs_build_tables",
    "pigs_path_upload", "pigs_path_download", "pigs_path_upload_all", "pigs_path_download_all",
    "pigs_delta_action_batch", "pigs_delta_action_batch_dev", "pigs_delta_action_parts",
    "pigs_commit_beads", "pigs_swap_tails", "pigs_potential_energy_slice",
    "pigs_therm_energy_batch", "pigs_local_energy_batch", "pigs_comm_unique_id",
    "pigs_comm_init_rank", "pigs_comm_init_all", "pigs_estimators_allreduce",
    "pigs_set_tuning", "pigs_selftest_fastmath", "pigs_selftest_stream_read", "pigs_selftest_log",
    "pigs_stage_reserve", "pigs_delta_action_staged", "pigs_commit_reserve", "pigs_commit_staged",
    "pigs_sampler_init", "pigs_sampler_seed", "pigs_sampler_set_rng", "pigs_sampler_get_rng", "pigs_sampler_step",
    "pigs_sampler_form", "pigs_sampler_counters", "pigs_sampler_counters16", "pigs_sampler_get_worm", "pigs_sampler_set_worm",
    "pigs_sampler_events", "pigs_sampler_event_ints", "pigs_sampler_nrho", "pigs_slice_download", "pigs_build_tables_kind", "pigs_structure_batch",
    "pigs_diagonal_estimators", "pigs_diagonal_estimators_begin", "pigs_diagonal_estimators_end",
    "pigs_density_init", "pigs_density_accumulate", "pigs_density_read",
    "pigs_fqt_init", "pigs_fqt_accumulate", "pigs_fqt_read",
    "pigs_sqv_init", "pigs_sqv_count", "pigs_sqv_vectors", "pigs_sqv_accumulate", "pigs_sqv_read",
    "pigs_fqv_init", "pigs_fqv_count", "pigs_fqv_vectors", "pigs_fqv_accumulate", "pigs_fqv_read",
    "pigs_fqs_init", "pigs_fqs_count", "pigs_fqs_vectors", "pigs_fqs_accumulate", "pigs_fqs_read",
    "pigs_grv_init", "pigs_grv_accumulate", "pigs_grv_read",
    "pigs_tau_init", "pigs_tau_accumulate", "pigs_tau_read",
    "pigs_bop_init", "pigs_bop_accumulate", "pigs_bop_read",
    "pigs_vh_init", "pigs_vh_accumulate", "pigs_vh_read",
    "pigs_g3_init", "pigs_g3_accumulate", "pigs_g3_read",
    "pigs_atm_init", "pigs_atm_accumulate", "pigs_atm_read",
    "pigs_nk_init", "pigs_nk_count", "pigs_nk_vectors", "pigs_nk_accumulate", "pigs_nk_add", "pigs_nk_read",
    "pigs_lat_init", "pigs_lat_accumulate", "pigs_lat_read",
    "pigs_sf_init", "pigs_sf_accumulate", "pigs_sf_read",
    "pigs_cl_np_max", "pigs_cl_init", "pigs_cl_accumulate", "pigs_cl_read", "pigs_cl_sweeps",
    "pigs_pc_np_max", "pigs_pc_init", "pigs_pc_accumulate", "pigs_pc_read", "pigs_pc_sweeps",
]


class PigsError(RuntimeError):
    pass


class PigsSweepParams(C.Structure):
    _fields_ = [("Nlev", C.c_int32), ("Nstag", C.c_int32), ("CMFreq", C.c_int32), ("Lstag", C.c_int32),
                ("delta_cm", C.c_double), ("CWorm", C.c_double), ("density", C.c_double), ("rbin", C.c_double),
                ("swapping", C.c_int32), ("Nobdm", C.c_int32), ("Nbin", C.c_int32), ("Npw", C.c_int32),
                ("sampling", C.c_int32), ("reserved", C.c_int32)]


class PigsParams(C.Structure):
    _fields_ = [("dim", C.c_int32), ("Np", C.c_int32), ("Nb", C.c_int32), ("Nmax", C.c_int32),
                ("trap", C.c_int32), ("wf_table", C.c_int32), ("v_table", C.c_int32),
                ("reserved", C.c_int32),
                ("dr", C.c_double), ("rcut2", C.c_double), ("dt", C.c_double), ("Rm", C.c_double),
                ("Lbox", C.c_double * 3), ("a_ho", C.c_double * 3)]


_lib = None


def load_library(path=LIB_PATH):
    """dlopen libpigs_hip.so (built in-tree by pathintegralgroundstate_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("PIGS_LIB", path)           # experiment builds (scripts/: e.g. the -DPIGS_SWEEP_TIMING library)
    if not os.path.exists(path):
        raise PigsError(
            f"{path} is missing: build it with `python -m pathintegralgroundstate_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.pigs_last_error.restype = C.c_char_p
    L.pigs_ctx_create.argtypes = [C.POINTER(PigsParams), _dp, _dp, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.pigs_ctx_destroy.argtypes = [vp]
    L.pigs_device_count.argtypes = [_ip]
    L.pigs_sync.argtypes = [vp]
    L.pigs_stream.argtypes = [vp, C.POINTER(vp)]
    L.pigs_build_tables.argtypes = [C.c_int32, C.c_double, C.c_double, _dp, _dp, _dp]
    L.pigs_build_tables_kind.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_double, _dp, _dp, _dp]
    L.pigs_path_upload.argtypes = [vp, C.c_int32, _dp]
    L.pigs_path_download.argtypes = [vp, C.c_int32, _dp]
    L.pigs_path_upload_all.argtypes = [vp, _dp]
    L.pigs_path_download_all.argtypes = [vp, _dp]
    L.pigs_delta_action_batch.argtypes = [vp, C.c_int64, _ip, _ip, _ip, _dp, _dp, _dp]
    L.pigs_delta_action_parts.argtypes = [vp, C.c_int64, _ip, _ip, _ip, _dp, _dp, _dp]
    L.pigs_delta_action_batch_dev.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.pigs_commit_beads.argtypes = [vp, C.c_int64, _ip, _ip, _ip, _dp]
    L.pigs_swap_tails.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.pigs_potential_energy_slice.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, _dp, _dp]
    L.pigs_therm_energy_batch.argtypes = [vp, C.c_int32, _ip, _dp, _dp, _dp]
    L.pigs_local_energy_batch.argtypes = [vp, C.c_int32, _ip, C.c_int32, _dp, _dp, _dp]
    L.pigs_comm_unique_id.argtypes = [C.c_char_p]
    L.pigs_comm_init_rank.argtypes = [vp, C.c_int32, C.c_int32, C.c_char_p]
    L.pigs_comm_init_all.argtypes = [C.POINTER(vp), C.c_int32]
    L.pigs_estimators_allreduce.argtypes = [vp, _dp, C.c_int32]
    L.pigs_stage_reserve.argtypes = [vp, C.c_int64, C.c_int64] + [C.POINTER(_ip)] * 3 + [C.POINTER(_dp)] * 3
    L.pigs_delta_action_staged.argtypes = [vp, C.c_int64]
    L.pigs_commit_reserve.argtypes = [vp, C.c_int64, C.c_int64] + [C.POINTER(_ip)] * 3 + [C.POINTER(_dp)]
    L.pigs_commit_staged.argtypes = [vp, C.c_int64]
    L.pigs_sampler_init.argtypes = [vp, C.POINTER(PigsSweepParams)]
    L.pigs_sampler_seed.argtypes = [vp, C.c_int32, C.c_int32]
    L.pigs_sampler_set_rng.argtypes = [vp, C.c_int32, C.c_int32, _ip]
    L.pigs_sampler_get_rng.argtypes = [vp, C.c_int32, _ip, _ip]
    L.pigs_sampler_step.argtypes = [vp, C.c_int32]
    L.pigs_sampler_form.argtypes = [vp, _ip]
    L.pigs_sampler_counters.argtypes = [vp, C.POINTER(C.c_int64)]
    L.pigs_sampler_counters16.argtypes = [vp, C.POINTER(C.c_int64)]
    L.pigs_sampler_get_worm.argtypes = [vp, _ip, _ip, _dp]
    L.pigs_sampler_set_worm.argtypes = [vp, _ip, _ip, _dp]
    L.pigs_sampler_events.argtypes = [vp, _ip]
    L.pigs_sampler_event_ints.argtypes = [vp, C.POINTER(C.c_int32)]
    L.pigs_sampler_nrho.argtypes = [vp, _dp, _ip]
    L.pigs_slice_download.argtypes = [vp, C.c_int32, _dp]
    L.pigs_structure_batch.argtypes = [vp, C.c_int32, _ip, C.c_int32, C.c_int32, C.c_double, C.c_int32, _dp, _dp]
    L.pigs_diagonal_estimators.argtypes = [vp, C.c_int32, _ip, C.c_int32, C.c_double, C.c_int32, _dp, _dp, _dp]
    L.pigs_diagonal_estimators_begin.argtypes = [vp, C.c_int32, _ip, C.c_int32, C.c_double, C.c_int32, C.c_int32]
    L.pigs_diagonal_estimators_end.argtypes = [vp, _dp, _dp, _dp]
    _lp = C.POINTER(C.c_int64)
    L.pigs_density_init.argtypes = [vp, C.c_int32, C.c_double]
    L.pigs_density_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_density_read.argtypes = [vp, _lp, _lp, _lp, _lp, _ip]
    L.pigs_fqt_init.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.pigs_fqt_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_fqt_read.argtypes = [vp, _dp, _lp, _ip]
    L.pigs_tau_init.argtypes = [vp]
    L.pigs_tau_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_tau_read.argtypes = [vp, _dp, _lp, _ip]
    L.pigs_sqv_init.argtypes = [vp, C.c_int32, C.c_int32]
    L.pigs_sqv_count.argtypes = [vp, _lp]
    L.pigs_sqv_vectors.argtypes = [vp, _ip]
    L.pigs_sqv_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_sqv_read.argtypes = [vp, _dp, _lp, _ip]
    L.pigs_fqv_init.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.pigs_fqv_count.argtypes = [vp, _lp]
    L.pigs_fqv_vectors.argtypes = [vp, _ip]
    L.pigs_fqv_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_fqv_read.argtypes = [vp, _dp, _lp, _ip]
    L.pigs_fqs_init.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.pigs_fqs_count.argtypes = [vp, _lp]
    L.pigs_fqs_vectors.argtypes = [vp, _ip]
    L.pigs_fqs_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_fqs_read.argtypes = [vp, _dp, _dp, _lp, _ip]
    L.pigs_grv_init.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int32]
    L.pigs_grv_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_grv_read.argtypes = [vp, _lp, _lp, _lp, _ip]
    L.pigs_bop_init.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double]
    L.pigs_bop_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_bop_read.argtypes = [vp, _dp, _lp, _dp, _lp, _lp, _ip]
    L.pigs_vh_init.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_double]
    L.pigs_vh_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_vh_read.argtypes = [vp, _lp, _lp, _lp, _ip]
    L.pigs_g3_init.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_int32]
    L.pigs_g3_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_g3_read.argtypes = [vp, _lp, _lp, _lp, _ip]
    L.pigs_atm_init.argtypes = [vp, C.c_double, C.c_int32]
    L.pigs_atm_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_atm_read.argtypes = [vp, _dp, _lp, _lp, _ip]
    L.pigs_nk_init.argtypes = [vp, C.c_int32, C.c_int32]
    L.pigs_nk_count.argtypes = [vp, _lp]
    L.pigs_nk_vectors.argtypes = [vp, _ip]
    L.pigs_nk_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_nk_add.argtypes = [vp, C.c_int32, _ip, _ip, _dp]
    L.pigs_nk_read.argtypes = [vp, _dp, _lp, _lp, _lp, _ip]
    L.pigs_lat_init.argtypes = [vp, C.c_int32, _dp, C.c_int32, C.c_double, C.c_int32, C.c_int32]
    L.pigs_lat_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_lat_read.argtypes = [vp, _dp, _lp, _lp, _lp, _lp, _lp, _lp, _lp, _lp, _ip]
    L.pigs_sf_init.argtypes = [vp, C.c_int32, C.c_int32]
    L.pigs_sf_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_sf_read.argtypes = [vp, _dp, _dp, _lp, _lp, _ip]
    L.pigs_cl_np_max.argtypes = []
    L.pigs_cl_init.argtypes = [vp, C.c_double, C.c_int32]
    L.pigs_cl_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_cl_read.argtypes = [vp, _lp, _lp, _lp, _lp, _dp, _ip]
    L.pigs_cl_sweeps.argtypes = [vp, C.POINTER(C.c_int32)]
    L.pigs_pc_np_max.argtypes = []
    L.pigs_pc_init.argtypes = [vp, C.c_double, C.c_int32, C.c_int32]
    L.pigs_pc_accumulate.argtypes = [vp, C.c_int32, _ip]
    L.pigs_pc_read.argtypes = [vp, _lp, _lp, _lp, _lp, _lp, _dp, _lp, _lp, _lp, _lp, _ip]
    L.pigs_pc_sweeps.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.pigs_set_tuning.argtypes = [vp, C.c_char_p, C.c_int32]
    L.pigs_selftest_fastmath.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
    L.pigs_selftest_stream_read.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pigs_selftest_log.argtypes = [vp, C.c_int64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    for name in ABI_SYMBOLS:
        fn = getattr(L, name)
        if name != "pigs_last_error":
            fn.restype = C.c_int
    _lib = L
    return L


def _chk(L, rc, what):
    if rc != 0:
        raise PigsError(f"{what} failed (status {rc}): {L.pigs_last_error().decode(errors='replace')}")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def _l(a):
    return a.ctypes.data_as(_lp)


_F, _N = np.float64, np.int64          # the two element types of the accumulator families (PigsContext._read)


def device_count():
    L = load_library()
    n = C.c_int32(0)
    rc = L.pigs_device_count(C.byref(n))
    return n.value if rc == 0 else 0


POTENTIALS = {"aziz2": 0, "lj": 1, "dipolar": 2}


def build_tables(cfg: SystemConfig, potential="aziz2"):
    """PotentialTable / JastrowTable (reference vpi_mod.f90:84-145) on the host."""
    L = load_library()
    VT = np.zeros(cfg.Nmax + 2)
    WF = np.zeros(cfg.Nmax + 2)
    dr = C.c_double()
    _chk(L, L.pigs_build_tables_kind(POTENTIALS[potential], cfg.Nmax, cfg.Rm, cfg.rcut, _d(VT), _d(WF),
                                     C.byref(dr)), "pigs_build_tables_kind")
    assert dr.value == cfg.dr
    return VT, WF


class PigsContext:
    """W resident walkers on one MI355X + the batched hot-path operations."""

    def __init__(self, cfg: SystemConfig, VTable, LogWF, n_walkers=1, device_id=0):
        self.L = load_library()
        self.cfg = cfg
        self.n_walkers = int(n_walkers)
        p = PigsParams()
        p.dim, p.Np, p.Nb, p.Nmax = cfg.dim, cfg.Np, cfg.Nb, cfg.Nmax
        p.trap, p.wf_table, p.v_table = int(cfg.trap), int(cfg.wf_table), int(cfg.v_table)
        p.dr, p.rcut2, p.dt, p.Rm = cfg.dr, cfg.rcut2, cfg.dt, cfg.Rm
        for k in range(3):
            p.Lbox[k] = cfg.Lbox[k]
            p.a_ho[k] = cfg.a_ho[k]
        self._VT = _f64(VTable)
        # wf_table = F (the reference's default): the trial function is evaluated analytically, LogWF may be None
        self._WF = _f64(LogWF) if LogWF is not None else np.zeros(cfg.Nmax + 2)
        if LogWF is None and cfg.wf_table:
            raise ValueError("wf_table = T needs a LogWF table")
        if self._VT.size != cfg.Nmax + 2 or self._WF.size != cfg.Nmax + 2:
            raise PigsError("tables must hold Nmax+2 doubles (F(0:Nmax+1))")
        h = C.c_void_p()
        _chk(self.L, self.L.pigs_ctx_create(C.byref(p), _d(self._VT), _d(self._WF), self.n_walkers,
                                            int(device_id), C.byref(h)), "pigs_ctx_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.pigs_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- residency
    def upload(self, walker, Path):
        Path = _f64(Path)
        assert Path.shape == self.cfg.path_shape, (Path.shape, self.cfg.path_shape)
        _chk(self.L, self.L.pigs_path_upload(self.h, int(walker), _d(Path)), "pigs_path_upload")

    def download(self, walker):
        Path = np.empty(self.cfg.path_shape)
        _chk(self.L, self.L.pigs_path_download(self.h, int(walker), _d(Path)), "pigs_path_download")
        return Path

    def upload_all(self, Paths):
        Paths = _f64(Paths)
        assert Paths.shape == (self.n_walkers,) + self.cfg.path_shape
        _chk(self.L, self.L.pigs_path_upload_all(self.h, _d(Paths)), "pigs_path_upload_all")

    def download_all(self):
        Paths = np.empty((self.n_walkers,) + self.cfg.path_shape)
        _chk(self.L, self.L.pigs_path_download_all(self.h, _d(Paths)), "pigs_path_download_all")
        return Paths

    def sync(self):
        _chk(self.L, self.L.pigs_sync(self.h), "pigs_sync")

    def stream(self):
        s = C.c_void_p()
        _chk(self.L, self.L.pigs_stream(self.h, C.byref(s)), "pigs_stream")
        return s.value

    def set_tuning(self, key, value):
        _chk(self.L, self.L.pigs_set_tuning(self.h, key.encode(), int(value)), "pigs_set_tuning")

    def selftest_fastmath(self, blocks=1024, iters=256):
        bad = (C.c_uint64 * 4)()
        _chk(self.L, self.L.pigs_selftest_fastmath(self.h, blocks, iters, bad), "pigs_selftest_fastmath")
        return list(bad), blocks * 256 * iters

    def selftest_log(self, n=1 << 30, seed=0x5eed):
        """(mismatches, one differing argument) of the sampler's device log against this host's libm on n arguments."""
        bad, x = C.c_uint64(), C.c_double()
        _chk(self.L, self.L.pigs_selftest_log(self.h, int(n), int(seed), C.byref(bad), C.byref(x)), "pigs_selftest_log")
        return bad.value, x.value

    def stream_read(self, reps=50):
        """(bytes, seconds) per plain streaming read of the resident worldlines (measurement aid)."""
        b, t = C.c_double(), C.c_double()
        _chk(self.L, self.L.pigs_selftest_stream_read(self.h, int(reps), C.byref(b), C.byref(t)), "pigs_selftest_stream_read")
        return b.value, t.value

    # ---- K1
    def delta_action_batch(self, walker, ip, ib, xnew, xold):
        """DeltaS[i] of moving bead ib[i] of particle ip[i] (1-based) of walker[i] from xold[i]
        to xnew[i]: UpdateAction's output (reference vpi_mod.f90:2491-2530) per item."""
        walker, ip, ib = _i32(walker).ravel(), _i32(ip).ravel(), _i32(ib).ravel()
        n = walker.size
        xnew, xold = _f64(xnew).reshape(n, self.cfg.dim), _f64(xold).reshape(n, self.cfg.dim)
        out = np.empty(n)
        _chk(self.L, self.L.pigs_delta_action_batch(self.h, n, _i(walker), _i(ip), _i(ib), _d(xnew),
                                                    _d(xold), _d(out)), "pigs_delta_action_batch")
        return out

    def delta_action_staged(self, walker, ip, ib, xnew, xold):
        """Same through the pinned staging arrays (the sampler's low-latency path)."""
        walker, ip, ib = _i32(walker).ravel(), _i32(ip).ravel(), _i32(ib).ravel()
        n, d = walker.size, self.cfg.dim
        pw, pp, pb = _ip(), _ip(), _ip()
        pxn, pxo, pds = _dp(), _dp(), _dp()
        _chk(self.L, self.L.pigs_stage_reserve(self.h, max(n, 1), 0, C.byref(pw), C.byref(pp), C.byref(pb),
                                               C.byref(pxn), C.byref(pxo), C.byref(pds)), "pigs_stage_reserve")
        np.ctypeslib.as_array(pw, (max(n, 1),))[:n] = walker
        np.ctypeslib.as_array(pp, (max(n, 1),))[:n] = ip
        np.ctypeslib.as_array(pb, (max(n, 1),))[:n] = ib
        np.ctypeslib.as_array(pxn, (max(n, 1) * d,))[:n * d] = _f64(xnew).ravel()
        np.ctypeslib.as_array(pxo, (max(n, 1) * d,))[:n * d] = _f64(xold).ravel()
        _chk(self.L, self.L.pigs_delta_action_staged(self.h, n), "pigs_delta_action_staged")
        return np.ctypeslib.as_array(pds, (max(n, 1),))[:n].copy()

    def commit_staged(self, walker, ip, ib, x):
        walker, ip, ib = _i32(walker).ravel(), _i32(ip).ravel(), _i32(ib).ravel()
        n, d = walker.size, self.cfg.dim
        pw, pp, pb, px = _ip(), _ip(), _ip(), _dp()
        _chk(self.L, self.L.pigs_commit_reserve(self.h, max(n, 1), 0, C.byref(pw), C.byref(pp), C.byref(pb),
                                                C.byref(px)), "pigs_commit_reserve")
        np.ctypeslib.as_array(pw, (max(n, 1),))[:n] = walker
        np.ctypeslib.as_array(pp, (max(n, 1),))[:n] = ip
        np.ctypeslib.as_array(pb, (max(n, 1),))[:n] = ib
        np.ctypeslib.as_array(px, (max(n, 1) * d,))[:n * d] = _f64(x).ravel()
        _chk(self.L, self.L.pigs_commit_staged(self.h, n), "pigs_commit_staged")
        self.sync()

    def delta_action_parts(self, walker, ip, ib, xnew, xold):
        """(DeltaPot, DeltaF2, DeltaLogPsi) per item: UpdatePot / UpdateWf outputs."""
        walker, ip, ib = _i32(walker).ravel(), _i32(ip).ravel(), _i32(ib).ravel()
        n = walker.size
        xnew, xold = _f64(xnew).reshape(n, self.cfg.dim), _f64(xold).reshape(n, self.cfg.dim)
        out = np.empty((n, 3))
        _chk(self.L, self.L.pigs_delta_action_parts(self.h, n, _i(walker), _i(ip), _i(ib), _d(xnew),
                                                    _d(xold), _d(out)), "pigs_delta_action_parts")
        return out

    def delta_action_batch_dev(self, n, d_walker, d_ip, d_ib, d_xnew, d_xold, d_out):
        """Device-pointer form (ints = raw device addresses), asynchronous on the context stream."""
        _chk(self.L, self.L.pigs_delta_action_batch_dev(self.h, int(n), d_walker, d_ip, d_ib, d_xnew,
                                                        d_xold, d_out), "pigs_delta_action_batch_dev")

    # ---- K6: device-resident sampler
    def sampler_init(self, Nlev=None, Nstag=None, CMFreq=None, Lstag=None, delta_cm=None, CWorm=0.0,
                     swapping=False, Nobdm=0, Nbin=None, Npw=0, sampling="bis"):
        c = self.cfg
        self._nbin = c.Nbin if Nbin is None else Nbin
        self._npw = Npw
        sp = PigsSweepParams(c.Nlev if Nlev is None else Nlev, c.Nstag if Nstag is None else Nstag,
                             c.CMFreq if CMFreq is None else CMFreq, c.Lstag if Lstag is None else Lstag,
                             c.delta_cm_eff if delta_cm is None else delta_cm, CWorm, c.density,
                             c.rcut / float(np.float32(self._nbin)), int(swapping), Nobdm, self._nbin, Npw,
                             {"bis": 0, "sta": 1}[sampling], 0)
        _chk(self.L, self.L.pigs_sampler_init(self.h, C.byref(sp)), "pigs_sampler_init")

    def sampler_seed(self, walker, seed):
        _chk(self.L, self.L.pigs_sampler_seed(self.h, int(walker), int(seed)), "pigs_sampler_seed")

    def sampler_set_rng(self, walker, mti, mt):
        mt = np.ascontiguousarray(mt, np.uint32).view(np.int32)
        _chk(self.L, self.L.pigs_sampler_set_rng(self.h, int(walker), int(mti), _i(mt)), "pigs_sampler_set_rng")

    def sampler_get_rng(self, walker):
        mti = C.c_int32()
        mt = np.zeros(624, np.int32)
        _chk(self.L, self.L.pigs_sampler_get_rng(self.h, int(walker), C.byref(mti), _i(mt)), "pigs_sampler_get_rng")
        return mti.value, mt.view(np.uint32).copy()

    def sampler_step(self, istep):
        _chk(self.L, self.L.pigs_sampler_step(self.h, int(istep)), "pigs_sampler_step")

    def sampler_form(self):
        """The form the sampler runs in: dict(sweep_threads, cm_H (workgroups per walker of the last step's TranslateChain
        kernel; 0: inside the sweep kernel, -1: no TranslateChain yet), stage_machine, cm_shared)."""
        out = np.zeros(4, np.int32)
        _chk(self.L, self.L.pigs_sampler_form(self.h, _i(out)), "pigs_sampler_form")
        return dict(sweep_threads=int(out[0]), cm_H=int(out[1]), stage_machine=bool(out[2]), cm_shared=bool(out[3]))

    def sampler_counters(self):
        acc = np.zeros((self.n_walkers, 4), np.int64)
        _chk(self.L, self.L.pigs_sampler_counters(self.h, acc.ctypes.data_as(C.POINTER(C.c_int64))),
             "pigs_sampler_counters")
        return acc

    def sampler_counters16(self):
        acc = np.zeros((self.n_walkers, 16), np.int64)
        _chk(self.L, self.L.pigs_sampler_counters16(self.h, acc.ctypes.data_as(C.POINTER(C.c_int64))),
             "pigs_sampler_counters16")
        return acc

    def sampler_get_worm(self):
        W, d = self.n_walkers, self.cfg.dim
        isopen, iworm, xend = np.zeros(W, np.int32), np.zeros(W, np.int32), np.zeros((W, 2, d))
        _chk(self.L, self.L.pigs_sampler_get_worm(self.h, _i(isopen), _i(iworm), _d(xend)), "pigs_sampler_get_worm")
        return isopen.astype(bool), iworm, xend

    def sampler_set_worm(self, isopen, iworm, xend):
        isopen, iworm, xend = _i32(isopen), _i32(iworm), _f64(xend)
        _chk(self.L, self.L.pigs_sampler_set_worm(self.h, _i(isopen), _i(iworm), _d(xend)), "pigs_sampler_set_worm")

    def sampler_events(self):
        n = C.c_int32()
        _chk(self.L, self.L.pigs_sampler_event_ints(self.h, C.byref(n)), "pigs_sampler_event_ints")
        ev = np.zeros((self.n_walkers, n.value), np.int32)
        _chk(self.L, self.L.pigs_sampler_events(self.h, _i(ev)), "pigs_sampler_events")
        return ev

    def sampler_nrho(self, reset=None):
        """nrho[w, ibin, l]; reset: None, True (all walkers) or a per-walker mask"""
        out = np.zeros((self.n_walkers, self._nbin, self._npw + 1))
        if reset is None or reset is False:
            keep, mask = None, None
        else:
            keep = np.ones(self.n_walkers, np.int32) if reset is True else _i32(reset)
            mask = _i(keep)
        _chk(self.L, self.L.pigs_sampler_nrho(self.h, _d(out), mask), "pigs_sampler_nrho")
        return out

    def slice_download(self, ib):
        R = np.empty((self.n_walkers, self.cfg.Np, self.cfg.dim))
        _chk(self.L, self.L.pigs_slice_download(self.h, int(ib), _d(R)), "pigs_slice_download")
        return R

    # ---- what the per-walker accumulator families below share
    def _accumulate(self, name, walkers):
        """pigs_<family>_accumulate `name` for `walkers` (None: all, the list left out)."""
        if walkers is None:
            _chk(self.L, getattr(self.L, name)(self.h, self.n_walkers, None), name)
        else:
            wl = _i32(walkers).ravel()
            _chk(self.L, getattr(self.L, name)(self.h, wl.size, _i(wl)), name)

    def _reset_mask(self, reset):
        """The `reset` of a *_read -- None, True (all walkers) or a per-walker mask -- as the library takes it: a
        pointer, which keeps its array alive, or None."""
        if reset is None or reset is False:
            return None
        keep = np.ones(self.n_walkers, np.int32) if reset is True else _i32(reset)
        if keep.size != self.n_walkers:
            raise ValueError("reset mask needs one entry per walker")
        return _i(keep)

    def _read(self, fam, state_attr, spec, reset):
        """pigs_<fam>_read.  `state_attr` names what <fam>_init leaves on this object (None: nothing), `spec(state)` lists
        (key, dtype, shape without the walker axis) in the order of the C arguments.  Returns the dict of those arrays;
        the walkers flagged by `reset` are zeroed after the copy."""
        state = None if state_attr is None else getattr(self, state_attr, None)
        if state_attr is not None and state is None:
            raise PigsError(f"{fam}_read: {fam}_init first")
        spec, name = spec(state), f"pigs_{fam}_read"
        out = {k: np.zeros((self.n_walkers,) + tuple(shape), dt) for k, dt, shape in spec}
        mask = self._reset_mask(reset)
        _chk(self.L, getattr(self.L, name)(self.h, *((_d if dt is _F else _l)(out[k]) for k, dt, _ in spec), mask), name)
        return out

    def _vectors(self, fam, nq):
        """pigs_<fam>_vectors: the stored vectors n [Nq, dim] (int32); `nq` is None before <fam>_init."""
        if nq is None:
            raise PigsError(f"{fam}_vectors: {fam}_init first")
        n, name = np.zeros((nq, self.cfg.dim), np.int32), f"pigs_{fam}_vectors"
        _chk(self.L, getattr(self.L, name)(self.h, _i(n)), name)
        return n

    # ---- density profiles of a trapped system (pigs_density_*: slice Nb, 64-bit counts per walker)
    def density_init(self, Nbin, half_width):
        """Allocate and zero the accumulators: Nbin bins per axis over [-half_width, half_width) (planar) and over
        [0, half_width) (radial, pair).  Calling it again resizes and zeroes them."""
        _chk(self.L, self.L.pigs_density_init(self.h, int(Nbin), float(half_width)), "pigs_density_init")
        self._dens_nbin = int(Nbin)

    def density_accumulate(self, walkers=None):
        """Queue one sample of slice Nb of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_density_accumulate", walkers)

    def density_read(self, reset=None):
        """dict of int64 arrays: planar [W, Nbin] (dim 1) or [W, Nbin, Nbin] (x fastest in the last axis), radial
        [W, Nbin], pair [W, Nbin], samples [W].  reset: None, True (all walkers) or a per-walker mask of walkers whose
        accumulators are zeroed after the copy."""
        dp = min(self.cfg.dim, 2)
        return self._read("density", "_dens_nbin", lambda nb: [
            ("planar", _N, (nb,) * dp), ("radial", _N, (nb,)), ("pair", _N, (nb,)), ("samples", _N, ())], reset)

    # ---- imaginary-time density correlations of a periodic system (pigs_fqt_*: raw sums per walker, lag, harmonic, axis)
    def fqt_init(self, Nk, Ntau, window):
        """Allocate and zero the sums of F(q, tau_l), l = 0..Ntau, over the slices Nb-window..Nb+window on the S(k) grid
        of Nk harmonics per axis.  The window has to stay inside the part of the path where the projection has
        converged; that is the caller's choice.  Calling it again resizes and zeroes."""
        _chk(self.L, self.L.pigs_fqt_init(self.h, int(Nk), int(Ntau), int(window)), "pigs_fqt_init")
        self._fqt_shape = (int(Ntau) + 1, int(Nk), self.cfg.dim)

    def fqt_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_fqt_accumulate", walkers)

    def fqt_read(self, reset=None):
        """dict: F, the raw sums [W, Ntau+1, Nk, dim] (profiles.normalize_fqt divides them), and samples [W] (int64).
        reset: None, True (all walkers) or a per-walker mask of walkers whose sums are zeroed after the copy."""
        return self._read("fqt", "_fqt_shape", lambda shape: [("F", _F, shape), ("samples", _N, ())], reset)

    # ---- imaginary-time profiles (pigs_tau_*: raw sums Vpair, Vext, W, D2 per walker and slice)
    def tau_init(self):
        """Allocate and zero the sums of the imaginary-time profiles (every slice b = 0..2Nb: pair and external potential
        energy, virial, squared link length).  Calling it again zeroes."""
        _chk(self.L, self.L.pigs_tau_init(self.h), "pigs_tau_init")

    def tau_accumulate(self, walkers=None):
        """Queue one sample of every slice of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_tau_accumulate", walkers)

    def tau_read(self, reset=None):
        """dict: Q, the raw sums [W, 2Nb+1, 4] (Vpair, Vext, W, D2; profiles.normalize_tau divides them), and samples [W]
        (int64).  reset: None, True (all walkers) or a per-walker mask of walkers whose sums are zeroed after the copy."""
        return self._read("tau", None, lambda _: [("Q", _F, (self.cfg.M, 4)), ("samples", _N, ())], reset)

    # ---- vector structure factor on the full reciprocal grid (pigs_sqv_*: raw sums per walker and vector)
    def sqv_init(self, nmax, window=0):
        """Allocate and zero the sums of S(q) over the slices Nb-window..Nb+window for the integer vectors |n_k| <= nmax
        of the half space (sqv_vectors lists them).  Calling it again resizes and zeroes."""
        _chk(self.L, self.L.pigs_sqv_init(self.h, int(nmax), int(window)), "pigs_sqv_init")
        nq = C.c_int64(0)
        _chk(self.L, self.L.pigs_sqv_count(self.h, C.byref(nq)), "pigs_sqv_count")
        self._sqv_nq = int(nq.value)

    def sqv_vectors(self):
        """The stored vectors n [Nq, dim] (int32) in the library's enumeration order."""
        return self._vectors("sqv", getattr(self, "_sqv_nq", None))

    def sqv_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_sqv_accumulate", walkers)

    def sqv_read(self, reset=None):
        """dict: S, the raw sums [W, Nq] (profiles.normalize_sqv divides them), and samples [W] (int64).
        reset: None, True (all walkers) or a per-walker mask of walkers whose sums are zeroed after the copy."""
        return self._read("sqv", "_sqv_nq", lambda nq: [("S", _F, (nq,)), ("samples", _N, ())], reset)

    # ---- F(q,tau) on the full reciprocal grid (pigs_fqv_*: raw sums per walker, lag and vector)
    def fqv_init(self, nmax, Ntau=0, window=0):
        """Allocate and zero the sums of F(q, tau_l), l = 0..Ntau, over the slices Nb-window..Nb+window for the vectors
        of sqv_init(nmax) (fqv_vectors lists them).  Lag 0 is sqv's S(q), bit for bit.  Calling it again resizes and
        zeroes."""
        _chk(self.L, self.L.pigs_fqv_init(self.h, int(nmax), int(Ntau), int(window)), "pigs_fqv_init")
        nq = C.c_int64(0)
        _chk(self.L, self.L.pigs_fqv_count(self.h, C.byref(nq)), "pigs_fqv_count")
        self._fqv_shape = (int(Ntau) + 1, int(nq.value))

    def fqv_vectors(self):
        """The stored vectors n [Nq, dim] (int32): those of sqv_vectors, in the same order."""
        return self._vectors("fqv", getattr(self, "_fqv_shape", (0, None))[1])

    def fqv_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_fqv_accumulate", walkers)

    def fqv_read(self, reset=None):
        """dict: F, the raw sums [W, Ntau+1, Nq] (profiles.normalize_fqv divides them), and samples [W] (int64).
        reset: None, True (all walkers) or a per-walker mask of walkers whose sums are zeroed after the copy."""
        return self._read("fqv", "_fqv_shape", lambda shape: [("F", _F, shape), ("samples", _N, ())], reset)

    # ---- self part of F(q,tau) and the imaginary-time displacement (pigs_fqs_*: raw sums per walker, lag and vector)
    def fqs_init(self, nmax, Ntau=0, window=0):
        """Allocate and zero the sums of the self part F_s(q, tau_l) and of the displacement |x_i(tau_l) - x_i(0)|^2,
        l = 0..Ntau, over the slices Nb-window..Nb+window for the vectors of sqv_init(nmax) (fqs_vectors lists them).
        Calling it again resizes and zeroes."""
        _chk(self.L, self.L.pigs_fqs_init(self.h, int(nmax), int(Ntau), int(window)), "pigs_fqs_init")
        nq = C.c_int64(0)
        _chk(self.L, self.L.pigs_fqs_count(self.h, C.byref(nq)), "pigs_fqs_count")
        self._fqs_shape = (int(Ntau) + 1, int(nq.value))

    def fqs_vectors(self):
        """The stored vectors n [Nq, dim] (int32): those of sqv_vectors, in the same order."""
        return self._vectors("fqs", getattr(self, "_fqs_shape", (0, None))[1])

    def fqs_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_fqs_accumulate", walkers)

    def fqs_read(self, reset=None):
        """dict: F, the raw sums [W, Ntau+1, Nq] (profiles.normalize_fqs divides them), D, the raw sums of r^2 and r^4
        [W, Ntau+1, 2] (profiles.normalize_msd), and samples [W] (int64).
        reset: None, True (all walkers) or a per-walker mask of walkers whose sums are zeroed after the copy."""
        return self._read("fqs", "_fqs_shape", lambda shape: [
            ("F", _F, shape), ("D", _F, (shape[0], 2)), ("samples", _N, ())], reset)

    # ---- pair distribution on the vector grid over a slice window (pigs_grv_*: 64-bit counts per walker)
    def grv_init(self, Nbin, window=0, Nr=None, rbin=None):
        """Allocate and zero the counts of g(r) over the slices Nb-window..Nb+window: Nbin bins per axis over the
        minimum-image cell, and Nr radial bins of width rbin (defaults: the context's Nbin and rcut / float32(Nbin), as
        sampler_init computes it).  Calling it again resizes and zeroes."""
        c = self.cfg
        nr = c.Nbin if Nr is None else int(Nr)
        rb = c.rcut / float(np.float32(nr)) if rbin is None else float(rbin)
        _chk(self.L, self.L.pigs_grv_init(self.h, int(Nbin), nr, rb, int(window)), "pigs_grv_init")
        self._grv_shape = (int(Nbin), nr)

    def grv_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_grv_accumulate", walkers)

    def grv_read(self, reset=None):
        """dict of int64 arrays: vec [W, Nbin, ..(dim times)] (x on the last axis), radial [W, Nr], samples [W]
        (profiles.normalize_grv turns them into g).  reset: None, True (all walkers) or a per-walker mask of walkers
        whose counts are zeroed after the copy."""
        dim = self.cfg.dim
        return self._read("grv", "_grv_shape", lambda shp: [
            ("vec", _N, (shp[0],) * dim), ("radial", _N, (shp[1],)), ("samples", _N, ())], reset)

    # ---- bond-orientational order over a slice window (pigs_bop_*: raw sums and 64-bit counts per walker)
    def bop_init(self, rnb, window=0, Nh=50, Nr=None, rbin=None):
        """Allocate and zero the accumulators of Q4, Q6 (2D: Psi_4, Psi_6), their local distributions in Nh bins over
        [0, 1] and G6(r) over the slices Nb-window..Nb+window of a periodic system in 2D or 3D; bonds are the pairs
        closer than rnb (at most half the shortest side).  Nr radial bins of width rbin (defaults: the context's Nbin
        and rcut / float32(Nbin), as grv_init); Nr = 0 switches G6(r) off.  Calling it again resizes and zeroes."""
        c = self.cfg
        nr = c.Nbin if Nr is None else int(Nr)
        rb = (c.rcut / float(np.float32(nr)) if nr > 0 else 0.0) if rbin is None else float(rbin)
        _chk(self.L, self.L.pigs_bop_init(self.h, float(rnb), int(window), int(Nh), nr, rb), "pigs_bop_init")
        self._bop_shape = (int(Nh), nr)

    def bop_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_bop_accumulate", walkers)

    def bop_read(self, reset=None):
        """dict: S [W, 8] (the sums of Q4, Q4^2, Q6, Q6^2, mean q4(i), mean q6(i), sum n_i, 0), H [W, 2, Nh] (int64), G
        [W, Nr], GN [W, Nr] (int64) and samples [W] (int64); profiles.normalize_bop divides them.  reset: None, True (all
        walkers) or a per-walker mask of walkers whose accumulators are zeroed after the copy."""
        return self._read("bop", "_bop_shape", lambda shp: [
            ("S", _F, (8,)), ("H", _N, (2, shp[0])), ("G", _F, (shp[1],)), ("GN", _N, (shp[1],)), ("samples", _N, ())], reset)

    # ---- van Hove functions over a slice window (pigs_vh_*: 64-bit counts per walker and lag)
    def vh_init(self, Ntau, window, Nr=None, rbin=None, Ns=50, sbin=None):
        """Allocate and zero the counts of the distinct and the self van Hove function for the lags 0..Ntau over the
        slices Nb-window..Nb+window of a periodic system: Nr radial bins of width rbin for |x_i(a+l) - x_j(a)|, i != j
        (defaults: the context's Nbin and rcut / float32(Nbin), as grv_init), and Ns bins of width sbin for the
        displacement |x_i(a+l) - x_i(a)| (default sbin: rcut / Ns).  Calling it again resizes and zeroes."""
        c = self.cfg
        nr = c.Nbin if Nr is None else int(Nr)
        rb = c.rcut / float(np.float32(nr)) if rbin is None else float(rbin)
        sb = c.rcut / float(Ns) if sbin is None else float(sbin)
        _chk(self.L, self.L.pigs_vh_init(self.h, int(Ntau), int(window), nr, rb, int(Ns), sb), "pigs_vh_init")
        self._vh_shape = (int(Ntau) + 1, nr, int(Ns))

    def vh_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_vh_accumulate", walkers)

    def vh_read(self, reset=None):
        """dict of int64 arrays: self [W, Ntau+1, Ns], distinct [W, Ntau+1, Nr], samples [W] (profiles.normalize_vh turns
        them into G_s and G_d).  reset: None, True (all walkers) or a per-walker mask of walkers whose counts are zeroed
        after the copy."""
        return self._read("vh", "_vh_shape", lambda shp: [
            ("self", _N, (shp[0], shp[2])), ("distinct", _N, (shp[0], shp[1])), ("samples", _N, ())], reset)

    # ---- triplet distribution over a slice window (pigs_g3_*: 64-bit counts per walker)
    def g3_init(self, Nr, rbin, Na, window=0):
        """Allocate and zero the counts of the triplet distribution over the slices Nb-window..Nb+window of a periodic 2D
        or 3D system: legs within rmax = Nr*rbin (at most half the shortest side) on Nr radial bins, the angle between two
        legs of a vertex on Na bins of cos(theta) over [-1, 1].  Calling it again resizes and zeroes."""
        _chk(self.L, self.L.pigs_g3_init(self.h, int(Nr), float(rbin), int(Na), int(window)), "pigs_g3_init")
        self._g3_shape = (int(Nr) * (int(Nr) + 1) // 2, int(Na), int(Nr))

    def g3_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_g3_accumulate", walkers)

    def g3_read(self, reset=None):
        """dict of int64 arrays: trip [W, Nr(Nr+1)/2, Na] on the packed upper triangle of leg-bin pairs (lo <= hi at
        lo*Nr - lo*(lo-1)/2 + hi - lo), pair [W, Nr], samples [W] (profiles.normalize_g3 turns them into g2 and g3).
        reset: None, True (all walkers) or a per-walker mask of walkers whose counts are zeroed after the copy."""
        return self._read("g3", "_g3_shape", lambda shp: [
            ("trip", _N, (shp[0], shp[1])), ("pair", _N, (shp[2],)), ("samples", _N, ())], reset)

    # ---- Axilrod-Teller-Muto three-body sum over a slice window (pigs_atm_*: a double and a 64-bit count per walker and slice)
    def atm_init(self, rc, window=0):
        """Allocate and zero the three-body sums over the slices Nb-window..Nb+window of a periodic 2D or 3D system: the
        triplets whose three nearest-image sides all lie within rc (at most half the shortest side).  Calling it again
        resizes and zeroes."""
        _chk(self.L, self.L.pigs_atm_init(self.h, float(rc), int(window)), "pigs_atm_init")
        self._atm_ns = 2 * int(window) + 1

    def atm_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_atm_accumulate", walkers)

    def atm_read(self, reset=None):
        """dict: T [W, 2 window + 1], the raw geometric sums of (1 + 3 cos cos cos)/(r r r)^3 (float64), ntrip, the
        triplets counted, of the same shape (int64), and samples [W] (int64); profiles.normalize_atm multiplies by the
        coupling and divides.  reset: None, True (all walkers) or a per-walker mask of walkers whose sums are zeroed
        after the copy."""
        return self._read("atm", "_atm_ns", lambda ns: [("T", _F, (ns,)), ("ntrip", _N, (ns,)), ("samples", _N, ())], reset)

    # ---- momentum distribution and one-body density matrix (pigs_nk_*: cosine sums per walker and vector, 64-bit counts)
    def nk_init(self, nmax, nbin):
        """Allocate and zero the sums of the momentum distribution of a periodic system on the vectors of sqv_init(nmax)
        (nk_vectors lists them) and the counts of the end-to-end vector on nbin bins per axis of the minimum-image cell.
        Calling it again resizes and zeroes."""
        _chk(self.L, self.L.pigs_nk_init(self.h, int(nmax), int(nbin)), "pigs_nk_init")
        nq = C.c_int64(0)
        _chk(self.L, self.L.pigs_nk_count(self.h, C.byref(nq)), "pigs_nk_count")
        self._nk = (int(nq.value), int(nbin))

    def nk_vectors(self):
        """The stored vectors n [Nq, dim] (int32) in the library's enumeration order (that of sqv_vectors)."""
        return self._vectors("nk", getattr(self, "_nk", (None,))[0])

    def nk_accumulate(self, walkers=None):
        """Queue the open-sector samples of the last sampler_step of `walkers` (None: all) on the context's stream; does
        not wait.  To be queued before the next step; a second call after the same step counts it again."""
        self._accumulate("pigs_nk_accumulate", walkers)

    def nk_add(self, walkers, nsamp, xend):
        """Add head/tail pairs from the host: nsamp[i] pairs for walkers[i] (None: walker i), xend [sum nsamp, 2, dim]
        (head, tail), the pairs of the first listed walker first.  Needs no sampler."""
        ns = _i32(nsamp).ravel()
        x = np.ascontiguousarray(xend, dtype=np.float64).reshape(-1)
        if x.size != int(ns.sum()) * 2 * self.cfg.dim:
            raise ValueError("xend needs 2*dim doubles per pair")
        if x.size == 0:
            x = np.zeros(1)
        if walkers is None:
            _chk(self.L, self.L.pigs_nk_add(self.h, ns.size, None, _i(ns), _d(x)), "pigs_nk_add")
        else:
            wl = _i32(walkers).ravel()
            if wl.size != ns.size:
                raise ValueError("one nsamp per listed walker")
            _chk(self.L, self.L.pigs_nk_add(self.h, wl.size, _i(wl), _i(ns), _d(x)), "pigs_nk_add")

    def nk_read(self, reset=None):
        """dict: C [W, Nq], the sums of cos(k.x) over the samples (float64), H [W, nbin, ..dim times] (array axis -1-k is
        axis k of the box), nopen [W] the samples (the sum of the vector n = 0) and ninside [W] those within rcut (int64);
        profiles.normalize_nk and normalize_nrvec divide them.  reset: None, True (all walkers) or a per-walker mask of
        walkers whose sums are zeroed after the copy."""
        dim = self.cfg.dim
        return self._read("nk", "_nk", lambda st: [
            ("C", _F, (st[0],)), ("H", _N, (st[1],) * dim), ("nopen", _N, ()), ("ninside", _N, ())], reset)

    # ---- a crystal seen from its lattice (pigs_lat_*: moments of the displacement from the nearest site, 64-bit counts)
    def lat_init(self, sites, nbin, rmax, window=0, cm=True):
        """Upload the lattice sites [nsite, dim] and allocate and zero the sums over the slices Nb-window..Nb+window of a
        periodic 2D or 3D system: nbin bins of |v| over [0, rmax) and 2 nbin bins of every v_k over [-rmax, rmax); cm:
        subtract the centre of mass of the displacements of every slice.  Calling it again resizes and zeroes."""
        R = np.ascontiguousarray(sites, dtype=np.float64)
        if R.ndim != 2 or R.shape[1] != self.cfg.dim:
            raise PigsError(f"lat_init: sites must be [nsite, {self.cfg.dim}]")
        if cm not in (0, 1, False, True):
            raise PigsError("lat_init: cm is 0 or 1")
        _chk(self.L, self.L.pigs_lat_init(self.h, R.shape[0], _d(R), int(nbin), float(rmax), int(window), int(cm)), "pigs_lat_init")
        self._lat = (2 * int(window) + 1, int(nbin))

    def lat_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_lat_accumulate", walkers)

    def lat_read(self, reset=None):
        """dict of the raw sums: mom [W, 2 window + 1, 2 + dim] (float64: sum |v|^2, sum |v|^4, sum v_k^2), and as int64
        nassigned [W, 2 window + 1], nlost [W], occ [W, 2 window + 1, 4] (sites with 0, 1, 2, >= 3 particles), hr [W, nbin],
        hx [W, dim, 2 nbin], hop1 [W], hopw [W], samples [W]; profiles.normalize_lat divides them.  reset: None, True (all
        walkers) or a per-walker mask of walkers whose sums are zeroed after the copy."""
        dim = self.cfg.dim
        return self._read("lat", "_lat", lambda st: [
            ("mom", _F, (st[0], 2 + dim)), ("nassigned", _N, (st[0],)), ("nlost", _N, ()), ("occ", _N, (st[0], 4)),
            ("hr", _N, (st[1],)), ("hx", _N, (dim, 2 * st[1])), ("hop1", _N, ()), ("hopw", _N, ()), ("samples", _N, ())], reset)

    # ---- the superfluid fraction from the centre-of-mass diffusion along tau (pigs_sf_*: raw sums per walker, lag and axis)
    def sf_init(self, Ntau=0, window=0):
        """Allocate and zero the sums of the squared unfolded displacement of the centre of mass (times Np) and of a
        particle over the lags l = 0..Ntau (0 <= Ntau <= 2 window), over the slices Nb-window..Nb+window of a periodic
        system.  Calling it again resizes and zeroes."""
        _chk(self.L, self.L.pigs_sf_init(self.h, int(Ntau), int(window)), "pigs_sf_init")
        self._sf = (int(Ntau) + 1, int(window))

    def sf_accumulate(self, walkers=None):
        """Queue one sample of the window of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_sf_accumulate", walkers)

    def sf_read(self, reset=None):
        """dict of the raw sums: C and D [W, Ntau+1, dim] (float64: the squared displacement over lag l of Np times the
        unfolded centre of mass, and of the unfolded particles), nwrap [W] (int64: the link components that were folded)
        and samples [W] (int64); and "window", the window they were taken over, which profiles.normalize_sf divides by.
        reset: None, True (all walkers) or a per-walker mask of walkers whose sums are zeroed after the copy."""
        dim = self.cfg.dim
        out = self._read("sf", "_sf", lambda st: [
            ("C", _F, (st[0], dim)), ("D", _F, (st[0], dim)), ("nwrap", _N, ()), ("samples", _N, ())], reset)
        out["window"] = self._sf[1]
        return out

    # ---- the cluster-size distribution over a slice window (pigs_cl_*: 64-bit counts and the sums of Rg^2 per walker and size)
    def cl_init(self, rc, window=0):
        """Allocate and zero the cluster sums of a periodic system: i and j are bonded iff 0 < r_ij^2 < rc^2 (minimum
        image, rc at most half the shortest side), a cluster is a connected component of that graph, over the slices
        Nb-window..Nb+window.  At most CL_NP_MAX particles.  Calling it again resizes and zeroes."""
        if self.cfg.Np > CL_NP_MAX:
            raise PigsError(f"cl_init: Np={self.cfg.Np} passes the {CL_NP_MAX} particles a workgroup labels")
        _chk(self.L, self.L.pigs_cl_init(self.h, float(rc), int(window)), "pigs_cl_init")
        self._cl = int(window)

    def cl_accumulate(self, walkers=None):
        """Queue one sample of every window slice of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_cl_accumulate", walkers)

    def cl_read(self, reset=None):
        """dict of the raw sums: nsize [W, Np] (int64: clusters of size s at s - 1), nlarge [W, Np] (int64: slices whose
        largest cluster has size s), nbond [W] and samples [W] (int64: bonds, and slices), rg2 [W, Np] (float64: the sum
        of the clusters' Rg^2 per size); and "window".  profiles.normalize_cl divides them.  reset: None, True (all
        walkers) or a per-walker mask of walkers whose sums are zeroed after the copy."""
        Np = self.cfg.Np
        out = self._read("cl", "_cl", lambda _: [
            ("nsize", _N, (Np,)), ("nlarge", _N, (Np,)), ("nbond", _N, ()), ("samples", _N, ()), ("rg2", _F, (Np,))], reset)
        out["window"] = self._cl
        return out

    def cl_sweeps(self):
        """The largest number of labelling sweeps any (walker, slice) needed since cl_init (a report, no result)."""
        v = C.c_int32(0)
        _chk(self.L, self.L.pigs_cl_sweeps(self.h, C.byref(v)), "pigs_cl_sweeps")
        return int(v.value)

    # ---- wrapping clusters, the finite clusters' unfolded Rg^2 and cluster persistence along tau (pigs_pc_*)
    def pc_init(self, rc, window=0, ntau=0):
        """Allocate and zero the percolation sums of a periodic system: cl_init's bonds and clusters over the slices
        Nb-window..Nb+window, and the persistence lags 0..ntau (at most 2 window).  At most CL_NP_MAX particles.  Works
        beside cl_init on the same context.  Calling it again resizes and zeroes."""
        if self.cfg.Np > CL_NP_MAX:
            raise PigsError(f"pc_init: Np={self.cfg.Np} passes the {CL_NP_MAX} particles a workgroup labels")
        _chk(self.L, self.L.pigs_pc_init(self.h, float(rc), int(window), int(ntau)), "pigs_pc_init")
        self._pc = (int(window), int(ntau))

    def pc_accumulate(self, walkers=None):
        """Queue one sample of every window slice of `walkers` (None: all) on the context's stream; does not wait."""
        self._accumulate("pigs_pc_accumulate", walkers)

    def pc_read(self, reset=None):
        """dict of the raw sums: nwrap, mwrap, swrap [W, 8] (int64, index = wrap mask: clusters, their particles, and slices
        by the OR of their clusters' masks), nfin [W, Np] (int64: finite clusters of size s at s - 1), samples [W] (int64:
        slices), rg2u [W, Np] (float64: the sum of the finite clusters' unfolded Rg^2 per size), first, second, both, norig
        [W, ntau + 1] (int64: pairs together in slice a, in a + l, in both, and the origins per lag); and "window", "ntau".
        profiles.normalize_pc divides them.  reset: None, True (all walkers) or a per-walker mask of walkers whose sums are
        zeroed after the copy."""
        Np = self.cfg.Np
        out = self._read("pc", "_pc", lambda st: [
            ("nwrap", _N, (8,)), ("mwrap", _N, (8,)), ("swrap", _N, (8,)), ("nfin", _N, (Np,)), ("samples", _N, ()),
            ("rg2u", _F, (Np,))] + [(k, _N, (st[1] + 1,)) for k in ("first", "second", "both", "norig")], reset)
        out["window"], out["ntau"] = self._pc
        return out

    def pc_sweeps(self):
        """(labelling sweeps, image-number sweeps): the largest counts any (walker, slice) needed since pc_init (a report,
        no result)."""
        a, b = C.c_int32(0), C.c_int32(0)
        _chk(self.L, self.L.pigs_pc_sweeps(self.h, C.byref(a), C.byref(b)), "pigs_pc_sweeps")
        return int(a.value), int(b.value)

    # ---- K5
    def commit_beads(self, walker, ip, ib, x):
        walker, ip, ib = _i32(walker).ravel(), _i32(ip).ravel(), _i32(ib).ravel()
        n = walker.size
        x = _f64(x).reshape(n, self.cfg.dim)
        _chk(self.L, self.L.pigs_commit_beads(self.h, n, _i(walker), _i(ip), _i(ib), _d(x)),
             "pigs_commit_beads")

    def swap_tails(self, walker, iw, ik):
        _chk(self.L, self.L.pigs_swap_tails(self.h, int(walker), int(iw), int(ik)), "pigs_swap_tails")

    # ---- K2..K4
    def potential_energy_slice(self, walker, ib, want_F2=False):
        p, f = C.c_double(), C.c_double()
        _chk(self.L, self.L.pigs_potential_energy_slice(self.h, int(walker), int(ib), int(want_F2),
                                                        C.byref(p), C.byref(f)),
             "pigs_potential_energy_slice")
        return p.value, f.value

    def therm_energy_batch(self, walkers=None):
        w = None if walkers is None else _i32(walkers).ravel()
        n = self.n_walkers if w is None else w.size
        E, Ec, Ep = np.empty(n), np.empty(n), np.empty(n)
        _chk(self.L, self.L.pigs_therm_energy_batch(self.h, n, None if w is None else _i(w), _d(E),
                                                    _d(Ec), _d(Ep)), "pigs_therm_energy_batch")
        return E, Ec, Ep

    def local_energy_batch(self, ib, walkers=None):
        w = None if walkers is None else _i32(walkers).ravel()
        n = self.n_walkers if w is None else w.size
        E, K, P = np.empty(n), np.empty(n), np.empty(n)
        _chk(self.L, self.L.pigs_local_energy_batch(self.h, n, None if w is None else _i(w), int(ib),
                                                    _d(E), _d(K), _d(P)), "pigs_local_energy_batch")
        return E, K, P

    # ---- K7
    def structure_batch(self, ib, Nbin, rbin, Nk, walkers=None):
        """(gr increments (n,Nbin), Sk increments (n,Nk,dim)) of slice ib: PairCorrelation and
        StructureFactor (reference sample_mod.f90:392-473)."""
        w = None if walkers is None else _i32(walkers).ravel()
        n = self.n_walkers if w is None else w.size
        gr = np.empty((n, Nbin))
        Sk = np.empty((n, Nk, self.cfg.dim))
        _chk(self.L, self.L.pigs_structure_batch(self.h, n, None if w is None else _i(w), int(ib), int(Nbin),
                                                 float(rbin), int(Nk), _d(gr), _d(Sk)), "pigs_structure_batch")
        return gr, Sk

    def diagonal_estimators(self, Nbin=0, rbin=0.0, Nk=0, walkers=None, structure=True):
        """All estimators of a diagonal MC step (vpi.f90:443-469) in one call: returns a dict with
        E1,K1,V1 (LocalEnergy slice 0), E2,K2,V2 (slice 2Nb), Et,Kt,Vt (ThermEnergy) -- arrays of n -- and, for PBC
        runs with structure=True, gr (n,Nbin), Sk (n,Nk,dim)."""
        w = None if walkers is None else _i32(walkers).ravel()
        n = self.n_walkers if w is None else w.size
        en = np.empty((n, 9))
        gr = Sk = None
        if structure and not self.cfg.trap:
            gr = np.empty((n, Nbin))
            Sk = np.empty((n, Nk, self.cfg.dim))
        _chk(self.L, self.L.pigs_diagonal_estimators(self.h, n, None if w is None else _i(w), int(Nbin), float(rbin), int(Nk),
                                                     _d(en), None if gr is None else _d(gr), None if Sk is None else _d(Sk)),
             "pigs_diagonal_estimators")
        out = {k: en[:, i] for i, k in enumerate(("E1", "K1", "V1", "E2", "K2", "V2", "Et", "Kt", "Vt"))}
        out["gr"], out["Sk"] = gr, Sk
        return out

    def diagonal_estimators_begin(self, Nbin=0, rbin=0.0, Nk=0, walkers=None, structure=True):
        """Asynchronous form: snapshot of the worldlines + estimator kernels on the context's second stream; go on (e.g.
        with the next sampler_step) and collect with diagonal_estimators_end()."""
        w = None if walkers is None else _i32(walkers).ravel()
        n = self.n_walkers if w is None else w.size
        st = bool(structure and not self.cfg.trap)
        self._est_pending = (n, int(Nbin), int(Nk), st)
        _chk(self.L, self.L.pigs_diagonal_estimators_begin(self.h, n, None if w is None else _i(w), int(Nbin), float(rbin),
                                                           int(Nk), int(st)), "pigs_diagonal_estimators_begin")

    def diagonal_estimators_end(self):
        n, Nbin, Nk, st = self._est_pending
        en = np.empty((n, 9))
        gr = np.empty((n, Nbin)) if st else None
        Sk = np.empty((n, Nk, self.cfg.dim)) if st else None
        _chk(self.L, self.L.pigs_diagonal_estimators_end(self.h, _d(en), None if gr is None else _d(gr),
                                                         None if Sk is None else _d(Sk)), "pigs_diagonal_estimators_end")
        out = {k: en[:, i] for i, k in enumerate(("E1", "K1", "V1", "E2", "K2", "V2", "Et", "Kt", "Vt"))}
        out["gr"], out["Sk"] = gr, Sk
        return out

    # ---- multi-GPU
    def comm_init_rank(self, nranks, rank, unique_id: bytes):
        _chk(self.L, self.L.pigs_comm_init_rank(self.h, nranks, rank, unique_id), "pigs_comm_init_rank")

    def estimators_allreduce(self, vec):
        vec = _f64(vec).copy()
        _chk(self.L, self.L.pigs_estimators_allreduce(self.h, _d(vec), vec.size),
             "pigs_estimators_allreduce")
        return vec

    # ---- reference-named single-call mirrors (argument meaning as in the reference) ----------
    def UpdateAction(self, walker, ip, ib, xnew, xold):
        """reference vpi_mod.f90:2491: DeltaS for one bead move."""
        return float(self.delta_action_batch([walker], [ip], [ib], [xnew], [xold])[0])

    def PotentialEnergy(self, walker, ib, want_F2=False):
        """reference sample_mod.f90:13: (Pot, F2) of slice ib."""
        return self.potential_energy_slice(walker, ib, want_F2)

    def LocalEnergy(self, walker, ib):
        """reference sample_mod.f90:154: (E, Kin, Pot) of slice ib."""
        E, K, P = self.local_energy_batch(ib, [walker])
        return float(E[0]), float(K[0]), float(P[0])

    def ThermEnergy(self, walker):
        """reference sample_mod.f90:323: (E, Ec, Ep) of one worldline."""
        E, Ec, Ep = self.therm_energy_batch([walker])
        return float(E[0]), float(Ec[0]), float(Ep[0])


def comm_unique_id():
    L = load_library()
    buf = C.create_string_buffer(128)
    _chk(L, L.pigs_comm_unique_id(buf), "pigs_comm_unique_id")
    return buf.raw
