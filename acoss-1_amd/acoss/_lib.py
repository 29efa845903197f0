"""ctypes binding of libacoss_hip.so (the C-ABI declared in include/acoss_hip.h).

This is the only door from Python into the HIP kernels. There is no CPU fallback: if the
library or a GPU is missing, every entry point raises ``AcossHipError``.

Device memory is owned by torch tensors; pointers go through ``Tensor.data_ptr()`` and
calls are ordered on the current torch stream.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ACOSS_HIP_LIB", os.path.join(_HERE, "lib", "libacoss_hip.so"))

ACOSS_OK = 0
_ERRNAMES = {-1: "ACOSS_E_ARG", -2: "ACOSS_E_SHAPE", -3: "ACOSS_E_HIP", -4: "ACOSS_E_NONBINARY"}


class AcossHipError(RuntimeError):
    """Raised on any failure of the HIP engine (missing library, no GPU, kernel error)."""


class CrpParams(ctypes.Structure):
    """acoss_crp_params — essentia ChromaCrossSimilarity/CoverSongSimilarity parameters
    (acoss/algorithms/rqa_serra09.py:31-32,60-64)."""
    _fields_ = [("m", ctypes.c_int32), ("tau", ctypes.c_int32), ("kappa", ctypes.c_float),
                ("oti", ctypes.c_int32), ("gamma_open", ctypes.c_float), ("gamma_ext", ctypes.c_float)]


BINARIZE = {"percentile": 0, "oti": 1}  # ACOSS_BIN_PERCENTILE, ACOSS_BIN_OTI


class CrpParams2(ctypes.Structure):
    """acoss_crp_params2 — acoss_crp_params and the binarisation (include/acoss_hip.h): what the
    entries ending in 2 take. m, tau, ... read through to the base."""
    _fields_ = [("base", CrpParams), ("binarize", ctypes.c_int32), ("oti_rank", ctypes.c_int32)]

    def __getattr__(self, name):  # only reached for what the struct itself does not have
        if name in ("m", "tau", "kappa", "oti", "gamma_open", "gamma_ext"):
            return getattr(self.base, name)
        raise AttributeError(name)


class CrpParams3(ctypes.Structure):
    """acoss_crp_params3 — acoss_crp_params2 and the ranked OTI (include/acoss_hip.h): what the entries
    ending in 3 take. n_oti is read by acoss_crp_align3 alone; oti_pick is the scalar pick of the
    others. m, tau, ..., binarize and oti_rank read through to the base."""
    _fields_ = [("base", CrpParams2), ("n_oti", ctypes.c_int32), ("oti_pick", ctypes.c_int32)]

    def __getattr__(self, name):  # only reached for what the struct itself does not have
        if name in ("m", "tau", "kappa", "oti", "gamma_open", "gamma_ext", "binarize", "oti_rank"):
            return getattr(self.base, name)
        raise AttributeError(name)


class NpzMember(ctypes.Structure):
    """acoss_npz_member — one array of an .npz feature file (include/acoss_hip.h)."""
    _fields_ = [("file", ctypes.c_int32), ("method", ctypes.c_int32), ("ndim", ctypes.c_int32),
                ("fortran", ctypes.c_int32), ("shape", ctypes.c_int64 * 8), ("nbytes", ctypes.c_int64),
                ("member_off", ctypes.c_int64), ("comp_size", ctypes.c_int64), ("npy_size", ctypes.c_int64),
                ("data_skip", ctypes.c_int64), ("name", ctypes.c_char * 128), ("descr", ctypes.c_char * 32)]


_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_f32 = ctypes.c_float

# name -> argtypes; every function returns int
SIGNATURES = {
    "acoss_crp_align": [_vp, _vp, _vp, _i32, _i32, _vp, _i64, ctypes.POINTER(CrpParams), _vp, _vp, _vp, _vp],
    "acoss_crp_pair": [_vp, _i32, _vp, _i32, ctypes.POINTER(CrpParams), _vp, _vp, _vp, _vp, _vp, _vp],
    "acoss_align_crp": [_vp, _i32, _i32, _i32, _f32, _f32, _vp, _vp],
    "acoss_crp_locate": [_vp, _vp, _vp, _i32, _i32, _vp, _i64, ctypes.POINTER(CrpParams), _vp, _vp, _vp, _vp],
    "acoss_locate_crp": [_vp, _i32, _i32, _f32, _f32, _vp, _vp, _vp],
    "acoss_crp_path": [_vp, _vp, _vp, _i32, _i32, _vp, _i64, ctypes.POINTER(CrpParams), _vp, _vp, _vp, _i32, _vp, _vp,
                       _vp],
    "acoss_path_crp": [_vp, _i32, _i32, _f32, _f32, _vp, _vp, _i32, _vp, _vp, _vp],
    "acoss_crp_locate_dmax": [_vp, _vp, _vp, _i32, _i32, _vp, _i64, ctypes.POINTER(CrpParams), _vp, _vp, _vp, _vp],
    "acoss_locate_crp_dmax": [_vp, _i32, _i32, _f32, _f32, _vp, _vp, _vp],
    "acoss_crp_path_dmax": [_vp, _vp, _vp, _i32, _i32, _vp, _i64, ctypes.POINTER(CrpParams), _vp, _vp, _vp, _i32, _vp,
                            _vp, _vp],
    "acoss_path_crp_dmax": [_vp, _i32, _i32, _f32, _f32, _vp, _vp, _i32, _vp, _vp, _vp],
    "acoss_crp_rqa": [_vp, _vp, _vp, _i32, _i32, _vp, _i64, ctypes.POINTER(CrpParams), _i32, _vp, _vp, _vp, _vp, _vp,
                      _i32, _vp, _vp],
    "acoss_rqa_crp": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "acoss_sw_constrained": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp],
    "acoss_sw_locate": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "acoss_sw_path": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp],
    "acoss_csm": [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp],
    "acoss_get_oti": [_vp, _vp, _i32, _vp, _vp],
    "acoss_binarize_rows": [_vp, _i32, _i32, _i32, _vp, _vp],
    "acoss_wcsm": [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp],
    "acoss_neg_exp": [_vp, _i64, _vp, _vp],
    "acoss_npz_index": [ctypes.POINTER(ctypes.c_char_p), _i32, ctypes.c_char_p, _i32, ctypes.POINTER(NpzMember), _i64,
                        ctypes.POINTER(ctypes.c_int64)],
    "acoss_npz_read": [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(NpzMember), _i64, ctypes.POINTER(_vp), _i32],
    "acoss_snf_step": [_vp, _i32, _i32, _i32, _vp, _vp, _i32, ctypes.c_double, _vp, _i32, _vp],
    "acoss_snf_diffuse_rows": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp],
    "acoss_snf_left_rows": [_vp, _i32, _i32, _i32, _vp, _vp, _i32, ctypes.c_double, _vp, _i32, _vp],
    "acoss_simple_mp": [_vp, _vp, _vp, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _vp],
    "acoss_simple_profile": [_vp, _vp, _vp, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "acoss_simple_self_profile": [_vp, _vp, _vp, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp,
                                  _vp],
    "acoss_median_downsample": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "acoss_simple_features": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i64, _vp],
    "acoss_earlyfusion": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, ctypes.c_double,
                          _i32, _f32, _vp, _vp],
    "acoss_earlyfusion_locate": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64,
                                 ctypes.c_double, _i32, _f32, _vp, _vp, _vp],
    "acoss_earlyfusion_path": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, ctypes.c_double,
                               _i32, _f32, _vp, _vp, _i32, _vp, _vp, _vp],
    "acoss_earlyfusion_snf": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, ctypes.c_double,
                              _i32, _f32, _i32, ctypes.c_double, _vp, _vp, _i64, _vp, _vp],
    "acoss_ef_block_features": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                _vp, _vp],
    "acoss_ftm2d_shingles": [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, ctypes.c_double, ctypes.c_double, _vp, _vp],
    "acoss_ftm2d_beatsync": [_vp, _vp, _vp, _i32, _vp, _vp, _i32, ctypes.c_double, _vp, _vp, _vp],
    "acoss_ftm2d_scores": [_vp, _i32, _i32, _vp, _i64, _vp, _vp],
    "acoss_ftm2d_topk": [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "acoss_ds_finish": [_vp, _i32, _i64, _vp, _i32, _i32, _vp, _vp],
    "acoss_eval_ranks": [_vp, _i32, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "acoss_release_workspace": [],
    "acoss_profile_enable": [ctypes.c_int],
    "acoss_profile_read": [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.c_int],
}
# the entries ending in 2: acoss_crp_params2 in place of acoss_crp_params, every other argument kept
# (acoss_crp_pair2 gains closer_out before the stream)
for _name in ("acoss_crp_align", "acoss_crp_locate", "acoss_crp_locate_dmax", "acoss_crp_path", "acoss_crp_path_dmax",
              "acoss_crp_rqa"):
    SIGNATURES[_name + "2"] = [ctypes.POINTER(CrpParams2) if a is ctypes.POINTER(CrpParams) else a
                               for a in SIGNATURES[_name]]
SIGNATURES["acoss_crp_pair2"] = [_vp, _i32, _vp, _i32, ctypes.POINTER(CrpParams2), _vp, _vp, _vp, _vp, _vp, _vp, _vp]
# the entries ending in 3: acoss_crp_params3, and the pick plane before the stream; acoss_crp_align3 has two
# shifts and two picks where acoss_crp_align2 has oti_out
for _name in ("acoss_crp_locate", "acoss_crp_locate_dmax", "acoss_crp_path", "acoss_crp_path_dmax", "acoss_crp_rqa"):
    SIGNATURES[_name + "3"] = [ctypes.POINTER(CrpParams3) if a is ctypes.POINTER(CrpParams) else a
                               for a in SIGNATURES[_name][:-1]] + [_vp, _vp]
SIGNATURES["acoss_crp_align3"] = [_vp, _vp, _vp, _i32, _i32, _vp, _i64, ctypes.POINTER(CrpParams3), _vp, _vp, _vp, _vp,
                                  _vp, _vp, _vp]
SIGNATURES["acoss_crp_pair3"] = [_vp, _i32, _vp, _i32, ctypes.POINTER(CrpParams3), _vp, _vp, _vp, _vp, _vp, _vp, _vp]
SIGNATURES["acoss_oti_ranked"] = [_vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp]
# EarlyFusion's entries ending in 2: int32 binarize (EF_BINARIZE) directly after mu; acoss_earlyfusion_snf2
# also gains binary_out before the stream
for _name in ("acoss_earlyfusion", "acoss_earlyfusion_locate", "acoss_earlyfusion_path", "acoss_earlyfusion_snf"):
    SIGNATURES[_name + "2"] = SIGNATURES[_name][:16] + [_i32] + SIGNATURES[_name][16:]
SIGNATURES["acoss_earlyfusion_snf2"] = SIGNATURES["acoss_earlyfusion_snf2"][:-1] + [_vp, _vp]
SIGNATURES["acoss_binarize_mutual"] = [_vp, _vp, _vp, _vp, _i32, _i32, _i32, ctypes.c_double, _i32, _vp, _vp]
EF_BINARIZE = {"rows": 0, "mutual": 1}  # ACOSS_EF_BIN_ROWS, ACOSS_EF_BIN_MUTUAL

_lib = None


def load_library(path=None):
    """Load (once) and return the ctypes handle. Raises AcossHipError if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise AcossHipError(
            "libacoss_hip.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C acoss-1_amd/csrc`). There is no CPU fallback." % p)
    # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's): load it first so
    # this library binds to the runtime torch's allocator and streams live in
    import torch  # noqa: F401
    lib = ctypes.CDLL(p)
    for name, argt in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argt
        fn.restype = ctypes.c_int
    lib.acoss_last_error.restype = ctypes.c_char_p
    lib.acoss_last_error.argtypes = []
    lib.acoss_version.restype = ctypes.c_char_p
    lib.acoss_version.argtypes = []
    lib.acoss_profile_phase_name.restype = ctypes.c_char_p
    lib.acoss_profile_phase_name.argtypes = [ctypes.c_int]
    if path is None:
        _lib = lib
    return lib


def _check(rc, what):
    if rc != ACOSS_OK:
        msg = load_library().acoss_last_error().decode(errors="replace")
        raise AcossHipError("%s failed (%s): %s" % (what, _ERRNAMES.get(rc, rc), msg))


_BOUND = [False]


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise AcossHipError("no HIP GPU visible to torch: the acoss HIP engine has no CPU fallback")
    if not _BOUND[0]:  # one process per GPU under RCCL: bind before the first "cuda" allocation
        from .distributed import bind_local_device
        _BOUND[0] = bind_local_device() is not None
    return torch


def _stream():
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(x, dtype):
    """numpy/torch -> contiguous device tensor of `dtype`."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        return x.to(device="cuda", dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype).contiguous()


def _check_pairs(pairs, n_tracks):
    """Host-side bounds check of (P, 2) track indices before a kernel dereferences them."""
    if pairs.numel() and (int(pairs.min()) < 0 or int(pairs.max()) >= n_tracks):
        raise ValueError("pair indices must lie in [0, %d)" % n_tracks)


def _pairs_dev(pairs, n_tracks):
    """(P, 2) int32 device pairs, bounds-checked. Host (numpy / list) pairs are checked on the
    host and uploaded from pinned memory without a stream synchronisation, so a caller feeding
    chunks keeps the GPU busy while it forms the next one; device tensors are checked on the
    device (two synchronising reductions). Returns (device tensor, host array or None)."""
    torch = _torch()
    if isinstance(pairs, torch.Tensor):
        d = pairs.to(device="cuda", dtype=torch.int32).reshape(-1, 2).contiguous()
        _check_pairs(d, n_tracks)
        return d, None
    h = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), dtype=np.int32)
    if len(h) and (int(h.min()) < 0 or int(h.max()) >= n_tracks):
        raise ValueError("pair indices must lie in [0, %d)" % n_tracks)
    if len(h) == 0:
        return torch.empty((0, 2), dtype=torch.int32, device="cuda"), h
    return torch.from_numpy(h).pin_memory().to("cuda", non_blocking=True), h


def check_knn(J, n):
    """Public form of the kNN index check (see snf_step(validated=True))."""
    _check_knn(J, n)


def _check_knn(J, n):
    """Host-side check of kNN column indices (n, K) before a kernel gathers the rows they name:
    every entry in [0, n), no repeated column within a row (scipy's coo -> csr would merge a
    repeat into one term, so the product would differ from the reference)."""
    if J.numel() == 0:
        return
    if int(J.min()) < 0 or int(J.max()) >= n:
        raise ValueError("kNN column indices must lie in [0, %d)" % n)
    if J.shape[1] > 1:
        Js = J.sort(dim=1).values
        if bool((Js[:, 1:] == Js[:, :-1]).any()):
            raise ValueError("kNN column indices repeat within a row")


def check_binarize(binarize, oti_rank):
    """The (binarize, oti_rank) every layer takes: 'percentile' (essentia's percentile CRP, oti_rank
    unused) or 'oti' (the OTI-binary CRP of Serra08, oti_rank in 1 .. 12; include/acoss_hip.h,
    acoss_crp_params2). Returns oti_rank as an int; raises ValueError otherwise."""
    if binarize not in BINARIZE:
        raise ValueError("binarize must be one of %s, not %r" % (", ".join(BINARIZE), binarize))
    if isinstance(oti_rank, bool) or int(oti_rank) != oti_rank or not 1 <= int(oti_rank) <= 12:
        raise ValueError("oti_rank must be an integer in 1 .. 12, not %r" % (oti_rank,))
    return int(oti_rank)


def binarize_suffix(binarize="percentile", oti_rank=1):
    """What a cache or result name carries for the binarisation: '' for the percentile CRP, '-otib'
    for the OTI-binary CRP at rank 1, '-otib<rank>' above."""
    oti_rank = check_binarize(binarize, oti_rank)
    if binarize == "percentile":
        return ""
    return "-otib" if oti_rank == 1 else "-otib%d" % oti_rank


def check_n_oti(n_oti, oti=True):
    """The n_oti every layer takes: how many of the ranked transpositions are aligned, the best kept
    (include/acoss_hip.h, acoss_crp_params3): an integer in 1 .. 12, and 1 without oti. Returns it as
    an int; raises ValueError otherwise."""
    if isinstance(n_oti, bool) or int(n_oti) != n_oti or not 1 <= int(n_oti) <= 12:
        raise ValueError("n_oti must be an integer in 1 .. 12, not %r" % (n_oti,))
    if int(n_oti) > 1 and not oti:
        raise ValueError("n_oti = %d needs oti=True: without the OTI there is no ranking" % int(n_oti))
    return int(n_oti)


def n_oti_suffix(n_oti=1, oti=True):
    """What a cache or result name carries for best of n: '' at 1, '-oti<n>' above. It follows the
    binarize suffix and precedes the measure: Serra09-otib2-oti2-det."""
    n_oti = check_n_oti(n_oti, oti)
    return "" if n_oti == 1 else "-oti%d" % n_oti


def crp_params3(params, n_oti=1, oti_pick=0):
    """acoss_crp_params3 around crp_params(...)'s struct: the crp_* calls below then take the entries
    ending in 3."""
    if isinstance(params, CrpParams3):
        params = params.base
    if not isinstance(params, CrpParams2):
        params = CrpParams2(params, BINARIZE["percentile"], 1)
    return CrpParams3(params, int(n_oti), int(oti_pick))


def crp_params(m=9, tau=1, kappa=0.095, oti=True, gamma_open=0.5, gamma_ext=0.5, binarize="percentile", oti_rank=1):
    """acoss_crp_params for the percentile CRP, acoss_crp_params2 for binarize='oti': the crp_* calls
    below pick the entry point (acoss_crp_align or acoss_crp_align2, ...) by the struct's type."""
    oti_rank = check_binarize(binarize, oti_rank)
    base = CrpParams(int(m), int(tau), float(kappa), int(bool(oti)), float(gamma_open), float(gamma_ext))
    return base if binarize == "percentile" else CrpParams2(base, BINARIZE[binarize], oti_rank)


def _entry(name, params):
    """The library entry `name` for these params: its twin ending in 2 for acoss_crp_params2, in 3
    for acoss_crp_params3."""
    return name + ("3" if isinstance(params, CrpParams3) else "2" if isinstance(params, CrpParams2) else "")


def _picked(params, picks, P):
    """(params, device pick plane or None) of a crp_locate / crp_path / crp_rqa call: a pick plane
    ((P,) int32, one rank of the ranked OTI per pair) takes the entry ending in 3."""
    if picks is None:
        return params, None
    torch = _torch()
    picks = _dev(picks, torch.int32).reshape(-1)
    if int(picks.shape[0]) != P:
        raise ValueError("picks has %d entries for %d pairs" % (int(picks.shape[0]), P))
    return (params if isinstance(params, CrpParams3) else crp_params3(params)), picks


def _n_pairs(pairs):
    """The number of pairs of a (P, 2) tensor, array or list."""
    if hasattr(pairs, "shape") and len(pairs.shape) == 2:
        return int(pairs.shape[0])
    return int(np.asarray(pairs).size // 2)


def oti_ranked(feats, track_off, track_len, pairs, dots=True):
    """The ranked OTI of every pair (acoss_oti_ranked): {"shifts" (P, 12) i32, the twelve shifts by
    descending profile dot, ties to the smaller shift, shifts[:, 0] the OTI; with dots "dots" (P, 12)
    f32, the dot of every shift}."""
    torch = _torch()
    feats = _dev(feats, torch.float32)
    track_off = _dev(track_off, torch.int64)
    track_len = _dev(track_len, torch.int32)
    pairs, _ = _pairs_dev(pairs, int(track_len.shape[0]))
    P = int(pairs.shape[0])
    out = {"shifts": _empty("int32", P, 12)}
    if dots:
        out["dots"] = _empty("float32", P, 12)
    rc = load_library().acoss_oti_ranked(_ptr(feats), _ptr(track_off), _ptr(track_len), int(track_len.shape[0]),
                                         _ptr(pairs), P, _ptr(out["shifts"]), _ptr(out.get("dots")), _stream())
    _check(rc, "acoss_oti_ranked")
    return out


# ----------------------------------------------------------------------------------------
# Thin wrappers: inputs/outputs are torch CUDA tensors.
# ----------------------------------------------------------------------------------------
def stacked_len(n, m=9, tau=1):
    """essentia stackChromaFrames count (common.hpp stacked_len)."""
    inc = m * tau
    return 0 if n <= inc else (n - inc + tau - 1) // tau


def _bank_args(feats, track_off, track_len, max_len, pairs, params):
    """What acoss_crp_align, acoss_crp_locate and acoss_crp_path take first: (device tensors to keep
    alive until the call is queued, P, the eight ctypes arguments up to params)."""
    torch = _torch()
    feats = _dev(feats, torch.float32)
    track_off = _dev(track_off, torch.int64)
    track_len = _dev(track_len, torch.int32)
    pairs, _ = _pairs_dev(pairs, int(track_len.shape[0]))
    P = int(pairs.shape[0])
    lead = (_ptr(feats), _ptr(track_off), _ptr(track_len), int(track_len.shape[0]), int(max_len), _ptr(pairs), P,
            ctypes.byref(params))
    return (feats, track_off, track_len, pairs), P, lead


def _matrix_args(C, gamma_open, gamma_ext):
    """What the given-matrix entries take: (C on the device as uint8, M, N, gamma_open, gamma_ext, stream)."""
    C = _dev(C, _torch().uint8)
    return C, int(C.shape[0]), int(C.shape[1]), float(gamma_open), float(gamma_ext), _stream()


def _empty(dtype, *shape):
    torch = _torch()
    return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")


def crp_align(feats, track_off, track_len, max_len, pairs, params, qmax=True, dmax=False, oti=False, n_oti=1):
    """Batched Serra09/Chen path. feats (sum_n, 12) f32, track_off (T,) i64, track_len (T,) i32,
    pairs (P, 2) i32 (query, reference) -> dict of device tensors.

    n_oti > 1, or acoss_crp_params3 for params: best of n_oti ranked transpositions
    (acoss_crp_align3). "qmax" / "dmax" are then the best scores, and each aligner asked for brings
    the shift and the pick that won it: "oti" and "pick_q" for Qmax (also with oti=True alone),
    "oti_d" and "pick_d" for dmax, (P,) i32 each."""
    if n_oti != 1:
        params = crp_params3(params, check_n_oti(n_oti, params.oti))
    if isinstance(params, CrpParams3):
        keep, P, lead = _bank_args(feats, track_off, track_len, max_len, pairs, params)
        out = {}
        if qmax or oti:
            out.update(oti=_empty("int32", P), pick_q=_empty("int32", P))
        if qmax:
            out["qmax"] = _empty("float32", P)
        if dmax:
            out.update(dmax=_empty("float32", P), oti_d=_empty("int32", P), pick_d=_empty("int32", P))
        rc = load_library().acoss_crp_align3(*lead, _ptr(out.get("qmax")), _ptr(out.get("dmax")), _ptr(out.get("oti")),
                                             _ptr(out.get("oti_d")), _ptr(out.get("pick_q")), _ptr(out.get("pick_d")),
                                             _stream())
        _check(rc, "acoss_crp_align3")
        return out
    keep, P, lead = _bank_args(feats, track_off, track_len, max_len, pairs, params)
    want = (("qmax", qmax, "float32"), ("dmax", dmax, "float32"), ("oti", oti, "int32"))
    out = {key: _empty(dtype, P) for key, on, dtype in want if on}
    entry = _entry("acoss_crp_align", params)
    rc = getattr(load_library(), entry)(*lead, _ptr(out.get("qmax")), _ptr(out.get("dmax")), _ptr(out.get("oti")),
                                        _stream())
    _check(rc, entry)
    return out


def crp_pair(X, Y, params, dist=True):
    """Single pair with intermediates: dist, thr_row, thr_col, crp (uint8), oti. Under binarize='oti'
    (acoss_crp_pair2) there are no thresholds: dist (D_0), crp, oti and closer (uint8, the count of
    transpositions strictly closer than the applied one)."""
    torch = _torch()
    lib = load_library()
    X = _dev(X, torch.float32)
    Y = _dev(Y, torch.float32)
    M, N = X.shape[0], Y.shape[0]
    Mp, Np = stacked_len(M, params.m, params.tau), stacked_len(N, params.m, params.tau)
    D = _empty("float32", Mp, Np) if dist else None
    if isinstance(params, (CrpParams2, CrpParams3)):  # acoss_crp_pair3: at the pick params.oti_pick
        entry = _entry("acoss_crp_pair", params)
        otib = params.binarize == BINARIZE["oti"]
        tr, tc = (None, None) if otib else (_empty("float32", Mp), _empty("float32", Np))
        C, o = _empty("uint8", Mp, Np), _empty("int32", 1)
        closer = _empty("uint8", Mp, Np) if otib else None
        rc = getattr(lib, entry)(_ptr(X), M, _ptr(Y), N, ctypes.byref(params), _ptr(D), _ptr(tr), _ptr(tc), _ptr(C),
                                 _ptr(o), _ptr(closer), _stream())
        _check(rc, entry)
        out = {"dist": D, "crp": C, "oti": o}
        out.update({"closer": closer} if otib else {"thr_row": tr, "thr_col": tc})
        return out
    tr, tc = _empty("float32", Mp), _empty("float32", Np)
    C, o = _empty("uint8", Mp, Np), _empty("int32", 1)
    rc = lib.acoss_crp_pair(_ptr(X), M, _ptr(Y), N, ctypes.byref(params), _ptr(D), _ptr(tr), _ptr(tc), _ptr(C),
                            _ptr(o), _stream())
    _check(rc, "acoss_crp_pair")
    return {"dist": D, "thr_row": tr, "thr_col": tc, "crp": C, "oti": o}


def align_crp(C, align=0, gamma_open=0.5, gamma_ext=0.5):
    """essentia CoverSongSimilarity(serra09|chen17, 'symmetric') on a binary (M, N) matrix."""
    C, M, N, go, ge, stream = _matrix_args(C, gamma_open, gamma_ext)
    out = _empty("float32", 1)
    rc = load_library().acoss_align_crp(_ptr(C), M, N, int(align), go, ge, _ptr(out), stream)
    _check(rc, "acoss_align_crp")
    return out


def score_key(align):
    """The result key of the score of the located / traced alignment: align 0 = serra09 ("qmax"), 1 = chen17 ("dmax")."""
    if align not in (0, 1):
        raise ValueError("align must be 0 (serra09, Qmax) or 1 (chen17, dmax)")
    return ("qmax", "dmax")[align]


def _aligner(align, name):
    """(result key of the score, library entry) of the Qmax (align = 0) or dmax (align = 1) form of `name`."""
    return score_key(align), name + ("_dmax" if align else "")


def dmax_path_bound(M, N):
    """The most cells a dmax (chen17) path of an (M, N) matrix can have: floor(2 (M + N) / 3) - 2 for
    M, N >= 3 (csrc/crp_internal.hpp dmax_path_bound has the proof). A Qmax path has at most min(M, N)."""
    return 0 if M < 3 or N < 3 else 2 * (M + N) // 3 - 2


def crp_locate(feats, track_off, track_len, max_len, pairs, params, align=0, picks=None):
    """Batched Qmax with its location (acoss_crp_locate): inputs as crp_align. Returns device tensors
    {"qmax" (P,) f32, "seg" (P, 4) i32 = (i0, j0, i1, j1) in stacked-frame rows / columns, (-1, -1, -1, -1)
    where Qmax is 0, "oti" (P,) i32}. align=1: the dmax (chen17) alignment instead
    (acoss_crp_locate_dmax), the score under "dmax"; its path may begin on an intermediate cell of a
    (2, 1) or (1, 2) step, so i0 or j0 may be 1 (see crp_path). picks ((P,) int32, or
    acoss_crp_params3 for params): the rank of the ranked OTI each pair is located at
    (acoss_crp_locate3); "oti" is the shift applied."""
    key, entry = _aligner(align, "acoss_crp_locate")
    params, picks = _picked(params, picks, _n_pairs(pairs))
    entry = _entry(entry, params)
    keep, P, lead = _bank_args(feats, track_off, track_len, max_len, pairs, params)
    out = {key: _empty("float32", P), "seg": _empty("int32", P, 4), "oti": _empty("int32", P)}
    tail = (_ptr(picks),) if isinstance(params, CrpParams3) else ()
    rc = getattr(load_library(), entry)(*lead, _ptr(out[key]), _ptr(out["seg"]), _ptr(out["oti"]), *tail, _stream())
    _check(rc, entry)
    return out


def locate_crp(C, gamma_open=0.5, gamma_ext=0.5, align=0):
    """Qmax of a binary (M, N) matrix and where it lies (acoss_locate_crp): (score (1,) f32,
    seg (4,) i32 = (i0, j0, i1, j1)) device tensors; the score is align_crp(C, 0, ...)'s. align=1:
    dmax and the chen17 alignment (acoss_locate_crp_dmax), the score align_crp(C, 1, ...)'s."""
    _, entry = _aligner(align, "acoss_locate_crp")
    C, M, N, go, ge, stream = _matrix_args(C, gamma_open, gamma_ext)
    out, seg = _empty("float32", 1), _empty("int32", 4)
    rc = getattr(load_library(), entry)(_ptr(C), M, N, go, ge, _ptr(out), _ptr(seg), stream)
    _check(rc, entry)
    return out, seg


PATH_CHUNK_BYTES = 1 << 30  # padded path output of one acoss_crp_path call (crp_path chunks its pairs by it)


def _compact_paths(lens, padded):
    """(P,) int32 lengths and (P, cap, 2) int32 padded paths -> the ragged form on the device:
    (path_off int64 (P + 1,), cells int32 (total, 2)); pair p owns cells[path_off[p]:path_off[p + 1]]."""
    torch = _torch()
    keep = torch.arange(padded.shape[1], device=padded.device, dtype=torch.int32)[None, :] < lens[:, None]
    off = torch.zeros(lens.shape[0] + 1, dtype=torch.int64, device=padded.device)
    off[1:] = torch.cumsum(lens.to(torch.int64), 0)
    return off, padded[keep].reshape(-1, 2)


def crp_path(feats, track_off, track_len, max_len, pairs, params, align=0, picks=None):
    """Batched Qmax with its whole alignment path (acoss_crp_path): inputs as crp_align. Returns device
    tensors {"qmax" (P,) f32, "seg" (P, 4) i32 and "oti" (P,) i32 as crp_locate, "path_off" (P + 1,)
    i64, "cells" (total, 2) i32}: the path of pair p is cells[path_off[p]:path_off[p + 1]], (i, j) in
    stacked-frame rows / columns from (i0, j0) to (i1, j1), empty where Qmax is 0. The pairs go to the
    library in chunks whose padded output stays near PATH_CHUNK_BYTES; each is compacted on the device.

    align=1: the dmax (chen17) alignment (acoss_crp_path_dmax), the score under "dmax". Its steps are
    (1, 1), (2, 1), (1, 2) and, exactly after the intermediate cell of a (2, 1) or (1, 2) step that
    is a hit, (1, 0) and (0, 1): non-decreasing in i and j, up to dmax_path_bound cells, and i0 or
    j0 may be 1 (a path may begin on such an intermediate cell, which may lie in row or column 1).
    picks: as crp_locate's (acoss_crp_path3)."""
    torch = _torch()
    lib = load_library()
    key, entry = _aligner(align, "acoss_crp_path")
    params, picks = _picked(params, picks, _n_pairs(pairs))
    entry = _entry(entry, params)
    keep, P, lead = _bank_args(feats, track_off, track_len, max_len, pairs, params)
    pairs = keep[3]
    L = stacked_len(int(max_len), params.m, params.tau)
    cap = max(1, dmax_path_bound(L, L) if align else L)
    q, seg, o = _empty("float32", P), _empty("int32", P, 4), _empty("int32", P)
    lens = _empty("int32", P)
    chunk = max(1, PATH_CHUNK_BYTES // (8 * cap))
    parts = []
    for a in range(0, P, chunk):
        n = min(chunk, P - a)
        padded = torch.empty((n, cap, 2), dtype=torch.int32, device="cuda")
        rc = getattr(lib, entry)(*lead[:5], _ptr(pairs[a:a + n]), int(n), lead[7], _ptr(q[a:a + n]),
                                 _ptr(seg[a:a + n]), _ptr(o[a:a + n]), int(cap), _ptr(lens[a:a + n]), _ptr(padded),
                                 *((_ptr(None if picks is None else picks[a:a + n]),)
                                   if isinstance(params, CrpParams3) else ()), _stream())
        _check(rc, entry)
        parts.append(_compact_paths(lens[a:a + n], padded)[1])
    off = torch.zeros(P + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens.to(torch.int64), 0)
    cells = torch.cat(parts) if parts else torch.empty((0, 2), dtype=torch.int32, device="cuda")
    return {key: q, "seg": seg, "oti": o, "path_off": off, "cells": cells}


def path_crp(C, gamma_open=0.5, gamma_ext=0.5, path_cap=None, align=0):
    """Qmax of a binary (M, N) matrix and its alignment path (acoss_path_crp): (score (1,) f32, seg (4,)
    i32, cells (len, 2) i32) device tensors; score and seg are locate_crp's. path_cap: entries of the
    padded buffer handed to the library, min(M, N) unless given (a smaller one is refused). align=1:
    dmax and the chen17 path (acoss_path_crp_dmax; steps and length as crp_path describes them),
    path_cap dmax_path_bound(M, N) unless given."""
    _, entry = _aligner(align, "acoss_path_crp")
    C, M, N, go, ge, stream = _matrix_args(C, gamma_open, gamma_ext)
    bound = dmax_path_bound(M, N) if align else min(M, N)
    cap = max(1, bound) if path_cap is None else int(path_cap)
    out, seg, n = _empty("float32", 1), _empty("int32", 4), _empty("int32", 1)
    padded = _empty("int32", max(1, cap), 2)
    rc = getattr(load_library(), entry)(_ptr(C), M, N, go, ge, _ptr(out), _ptr(seg), cap, _ptr(n), _ptr(padded),
                                        stream)
    _check(rc, entry)
    return out, seg, padded[:int(n.item())]


RQA_COUNTS = ("n_rec", "n_lines", "n_lines_min", "n_pts_min")  # columns of "counts"
RQA_STATS = ("rr", "det", "lmean", "entr")                      # columns of "stats"


def crp_rqa(feats, track_off, track_len, max_len, pairs, params, lmin=2, smax=True, hist_cap=0, lines=True,
            picks=None):
    """Batched cross-recurrence quantification (acoss_crp_rqa; the definition: include/acoss_hip.h):
    inputs as crp_align. Returns device tensors {"counts" (P, 4) i64 = RQA_COUNTS, "lmax" (P,) i32,
    "stats" (P, 4) f64 = RQA_STATS, "oti" (P,) i32, with smax "smax" (P,) f32, with hist_cap > 0
    "hist" (P, hist_cap) i32, hist[p, l] = the number of diagonal lines of length l}. lines=False
    leaves "counts", "lmax" and "stats" out and skips the line walk unless a histogram is asked for.
    picks: as crp_locate's (acoss_crp_rqa3)."""
    params, picks = _picked(params, picks, _n_pairs(pairs))
    keep, P, lead = _bank_args(feats, track_off, track_len, max_len, pairs, params)
    out = {"oti": _empty("int32", P)}
    if lines:
        out.update(counts=_empty("int64", P, 4), lmax=_empty("int32", P), stats=_empty("float64", P, 4))
    if smax:
        out["smax"] = _empty("float32", P)
    if hist_cap:
        out["hist"] = _empty("int32", P, int(hist_cap))
    entry = _entry("acoss_crp_rqa", params)
    rc = getattr(load_library(), entry)(*lead, int(lmin), _ptr(out.get("counts")), _ptr(out.get("lmax")),
                                        _ptr(out.get("stats")), _ptr(out.get("smax")), _ptr(out["oti"]), int(hist_cap),
                                        _ptr(out.get("hist")),
                                        *((_ptr(picks),) if isinstance(params, CrpParams3) else ()), _stream())
    _check(rc, entry)
    return out


def rqa_crp(C, lmin=2, smax=True, hist=False):
    """Cross-recurrence quantification of a binary (M, N) matrix (acoss_rqa_crp): device tensors
    {"counts" (4,) i64, "lmax" (1,) i32, "stats" (4,) f64, with smax "smax" (1,) f32, with hist
    "hist" i32}. hist=True returns every bin, min(M, N) + 1 entries; an integer the first that many."""
    C, M, N, _, _, stream = _matrix_args(C, 0.0, 0.0)
    cap = 0 if hist is False else (min(M, N) + 1 if hist is True else int(hist))
    out = {"counts": _empty("int64", 4), "lmax": _empty("int32", 1), "stats": _empty("float64", 4)}
    if smax:
        out["smax"] = _empty("float32", 1)
    if cap:
        out["hist"] = _empty("int32", cap)
    rc = load_library().acoss_rqa_crp(_ptr(C), M, N, int(lmin), _ptr(out["counts"]), _ptr(out["lmax"]),
                                      _ptr(out["stats"]), _ptr(out.get("smax")), cap, _ptr(out.get("hist")), stream)
    _check(rc, "acoss_rqa_crp")
    return out


def _pack_mats(mats, dtype):
    """list of 2-D arrays -> (flat device buffer, offsets i64, rows i32, cols i32, max_rows, max_cols)."""
    torch = _torch()
    shapes = [tuple(int(v) for v in m.shape) for m in mats]
    sizes = [r * c for r, c in shapes]
    off = np.zeros(len(mats), dtype=np.int64)
    if len(mats) > 1:
        off[1:] = np.cumsum(sizes[:-1])
    flat = torch.empty(max(1, int(sum(sizes))), dtype=dtype, device="cuda")
    for m, o, n in zip(mats, off, sizes):
        if n:
            flat[int(o):int(o) + n] = _dev(m, dtype).reshape(-1)
    rows = np.array([r for r, _ in shapes], dtype=np.int32)
    cols = np.array([c for _, c in shapes], dtype=np.int32)
    return (flat, _dev(off, torch.int64), _dev(rows, torch.int32), _dev(cols, torch.int32),
            int(rows.max(initial=0)), int(cols.max(initial=0)))


def _as_binary_u8(m):
    """Binary matrix -> uint8, raising like `match` (alignment_tools.py:17-23) on other values."""
    torch = _torch()
    t = m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m))
    if t.dtype not in (torch.uint8, torch.bool):
        t = t.to("cuda")
        if bool(((t != 0) & (t != 1)).any()):
            raise IOError("Non-binary elements found in input")
    return t.to(device="cuda", dtype=torch.uint8)


def sw_constrained(mats):
    """smith_waterman_constrained (alignment_tools.py:27-46) of a list of binary matrices -> (n,) f64."""
    torch = _torch()
    lib = load_library()
    mats = [_as_binary_u8(m) for m in mats]
    out = torch.empty(len(mats), dtype=torch.float64, device="cuda")
    if not mats:
        return out
    flat, off, rows, cols, mr, mc = _pack_mats(mats, torch.uint8)
    rc = lib.acoss_sw_constrained(_ptr(flat), _ptr(off), _ptr(rows), _ptr(cols), len(mats), mr, mc, _ptr(out),
                                  _stream())
    if rc == -4:
        raise IOError("Non-binary elements found in input")
    _check(rc, "acoss_sw_constrained")
    return out


CSM_KINDS = {"euclidean": 0, "euclid": 0, "cosine": 1, "ssm": 2}


def sw_path_bound(M, N):
    """The most cells a constrained Smith-Waterman path of an (M, N) matrix can have: its cells lie in
    [2, M - 2] x [2, N - 2] and climb in both coordinates (include/acoss_hip.h, acoss_sw_locate)."""
    return max(0, min(int(M), int(N)) - 3)


def sw_locate(mats):
    """smith_waterman_constrained of a list of binary matrices with where its alignment lies
    (acoss_sw_locate): device tensors {"score" (n,) f64, sw_constrained's bit for bit, "seg" (n, 4) i32 =
    (r0, c0, r1, c1), the first and last cell of the path in the matrix's own rows and columns,
    (-1, -1, -1, -1) where the score is 0}."""
    torch = _torch()
    mats = [_as_binary_u8(m) for m in mats]
    out = {"score": _empty("float64", len(mats)), "seg": _empty("int32", len(mats), 4)}
    if not mats:
        return out
    flat, off, rows, cols, mr, mc = _pack_mats(mats, torch.uint8)
    rc = load_library().acoss_sw_locate(_ptr(flat), _ptr(off), _ptr(rows), _ptr(cols), len(mats), mr, mc,
                                        _ptr(out["score"]), _ptr(out["seg"]), _stream())
    if rc == -4:
        raise IOError("Non-binary elements found in input")
    _check(rc, "acoss_sw_locate")
    return out


def sw_path(mats, path_cap=None):
    """sw_locate with the whole path (acoss_sw_path): {"score", "seg", "path_off" (n + 1,) i64, "cells"
    (total, 2) i32}; the path of matrix k is cells[path_off[k]:path_off[k + 1]], (r, c) from (r0, c0)
    to (r1, c1) in steps (1, 1), (2, 1), (1, 2), empty where the score is 0. path_cap: entries per
    matrix of the padded buffer handed to the library, sw_path_bound of the largest rows and columns
    unless given (a smaller one is refused). The matrices go to the library in chunks whose padded
    output and direction planes stay near PATH_CHUNK_BYTES; each is compacted on the device."""
    torch = _torch()
    lib = load_library()
    mats = [_as_binary_u8(m) for m in mats]
    n = len(mats)
    score, seg, lens = _empty("float64", n), _empty("int32", n, 4), _empty("int32", n)
    mr = max([int(m.shape[0]) for m in mats], default=0)
    mc = max([int(m.shape[1]) for m in mats], default=0)
    cap = max(1, sw_path_bound(mr, mc)) if path_cap is None else int(path_cap)
    chunk = max(1, PATH_CHUNK_BYTES // (8 * max(1, cap) + mr * mc // 4 + 1))
    parts = []
    for a in range(0, n, chunk):
        k = min(chunk, n - a)
        flat, off, rows, cols, _, _ = _pack_mats(mats[a:a + k], torch.uint8)
        padded = torch.empty((k, max(1, cap), 2), dtype=torch.int32, device="cuda")
        rc = lib.acoss_sw_path(_ptr(flat), _ptr(off), _ptr(rows), _ptr(cols), k, mr, mc, _ptr(score[a:a + k]),
                               _ptr(seg[a:a + k]), cap, _ptr(lens[a:a + k]), _ptr(padded), _stream())
        if rc == -4:
            raise IOError("Non-binary elements found in input")
        _check(rc, "acoss_sw_path")
        parts.append(_compact_paths(lens[a:a + k], padded)[1])
    path_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    path_off[1:] = torch.cumsum(lens.to(torch.int64), 0)
    cells = torch.cat(parts) if parts else torch.empty((0, 2), dtype=torch.int32, device="cuda")
    return {"score": score, "seg": seg, "path_off": path_off, "cells": cells}


def csm(X, Y=None, kind="euclidean", oti_shift=0):
    """get_csm / get_csm_cosine / get_ssm (cross_recurrence.py:10-73); oti_shift > 0 rolls each
    12-bin block of X first (get_csm_blocked_oti, :105-134). float32 (M, N) device tensor."""
    torch = _torch()
    lib = load_library()
    k = CSM_KINDS[kind]
    X = _dev(X, torch.float32)
    if X.dim() != 2:
        raise ValueError("X must be 2-D")
    if k == 2:
        Yt, N = None, X.shape[0]
    else:
        Yt = _dev(Y, torch.float32)
        if Yt.dim() != 2 or Yt.shape[1] != X.shape[1]:
            raise ValueError("X and Y need the same feature dimension")
        N = Yt.shape[0]
    out = torch.empty((X.shape[0], N), dtype=torch.float32, device="cuda")
    rc = lib.acoss_csm(_ptr(X), int(X.shape[0]), _ptr(Yt), int(N), int(X.shape[1]), k, int(oti_shift), _ptr(out),
                       _stream())
    _check(rc, "acoss_csm")
    return out


def get_oti(C1, C2):
    """get_oti (cross_recurrence.py:75-103) for (n, 12) batches (or single (12,) vectors)."""
    torch = _torch()
    lib = load_library()
    a = _dev(C1, torch.float32).reshape(-1, 12)
    b = _dev(C2, torch.float32).reshape(-1, 12)
    out = torch.empty(a.shape[0], dtype=torch.int32, device="cuda")
    rc = lib.acoss_get_oti(_ptr(a), _ptr(b), int(a.shape[0]), _ptr(out), _stream())
    _check(rc, "acoss_get_oti")
    return out


def binarize_rows(D, nneighbs):
    """The nneighbs smallest of every row -> 1 (csm_to_binary, cross_recurrence.py:136-161)."""
    torch = _torch()
    lib = load_library()
    D = _dev(D, torch.float32)
    out = torch.empty(D.shape, dtype=torch.uint8, device="cuda")
    rc = lib.acoss_binarize_rows(_ptr(D), int(D.shape[0]), int(D.shape[1]), int(nneighbs), _ptr(out), _stream())
    _check(rc, "acoss_binarize_rows")
    return out


def binarize_mutual(mats, kappa, mutual=True):
    """The binarisation of EarlyFusion alone (acoss_binarize_mutual; "mutual" in include/acoss_hip.h)
    for a list of float32 matrices: a list of uint8 device tensors of the same shapes, the mutual
    rule, or the row rule csm_to_binary computes (mutual=False). It runs the batched pipeline's own
    kernels; the largest row and column count of the list pick the shape class, as max_blocks does
    there. Counts are clamped to the line lengths (no ValueError here)."""
    binarize = check_ef_binarize(mutual)
    if not kappa >= 0:
        raise ValueError("kappa must be >= 0, got %r" % (kappa,))
    torch = _torch()
    mats = [_dev(m, torch.float32) for m in mats]
    if any(m.dim() != 2 or m.shape[0] < 1 or m.shape[1] < 1 for m in mats):
        raise ValueError("binarize_mutual takes non-empty 2-D matrices")
    if not mats:
        return []
    flat, off, rows, cols, mr, mc = _pack_mats(mats, torch.float32)
    out = torch.empty(flat.shape[0], dtype=torch.uint8, device="cuda")
    rc = load_library().acoss_binarize_mutual(_ptr(flat), _ptr(off), _ptr(rows), _ptr(cols), len(mats), mr, mc,
                                              float(kappa), binarize, _ptr(out), _stream())
    _check(rc, "acoss_binarize_mutual")
    offs = off.cpu().numpy()
    return [out[int(o):int(o) + m.numel()].reshape(m.shape) for o, m in zip(offs, mats)]


def wcsm(CSM, k1, k2, mu=0.5):
    """getWCSM (similarity_fusion.py:38-54)."""
    torch = _torch()
    lib = load_library()
    C = _dev(CSM, torch.float32)
    out = torch.empty(C.shape, dtype=torch.float32, device="cuda")
    rc = lib.acoss_wcsm(_ptr(C), int(C.shape[0]), int(C.shape[1]), int(k1), int(k2), float(mu), _ptr(out), _stream())
    _check(rc, "acoss_wcsm")
    return out


def npz_read_many(paths, keys=None, n_threads=0):
    """The arrays of many .npz files, read on native threads in two C calls (acoss_npz_index,
    acoss_npz_read; host only, no GPU, the GIL released inside both): a list (one per path, in
    order) of {member name: ndarray}, names as stored ('madmom_features/onsets'). keys: read only
    members whose top-level name is in keys (None: all). Raises IOError naming the file on an
    unreadable or unsupported file (object arrays are refused, as np.load(allow_pickle=False))."""
    lib = load_library()
    n = len(paths)
    if n == 0:
        return []
    cpaths = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
    ckeys = None if keys is None else "\n".join(keys).encode()
    cap = max(16, n * (4 if keys is not None else 8))
    while True:
        buf = (NpzMember * cap)()
        got = ctypes.c_int64(0)
        rc = lib.acoss_npz_index(cpaths, n, ckeys, int(n_threads), buf, cap, ctypes.byref(got))
        if rc == ACOSS_OK:
            break
        if got.value > cap:
            cap = int(got.value)
            continue
        raise IOError(lib.acoss_last_error().decode(errors="replace"))
    members = buf[:got.value]
    out = [dict() for _ in range(n)]
    arrays = []
    for m in members:
        shape = tuple(int(m.shape[d]) for d in range(m.ndim))
        a = np.empty(shape, dtype=np.dtype(m.descr.decode()), order="F" if m.fortran else "C")
        arrays.append(a)
        out[m.file][m.name.decode()] = a
    if members:
        dst = (_vp * len(members))(*[a.ctypes.data for a in arrays])
        rc = lib.acoss_npz_read(cpaths, buf, len(members), dst, int(n_threads))
        if rc != ACOSS_OK:
            raise IOError(lib.acoss_last_error().decode(errors="replace"))
    return out


def neg_exp(x):
    """exp(-x) elementwise in the canonical float32 exp (acoss_neg_exp; the early matrix of
    EarlyFusion, earlyfusion_traile.py:182)."""
    torch = _torch()
    lib = load_library()
    X = _dev(x, torch.float32)
    out = torch.empty(X.shape, dtype=torch.float32, device="cuda")
    rc = lib.acoss_neg_exp(_ptr(X), int(X.numel()), _ptr(out), _stream())
    _check(rc, "acoss_neg_exp")
    return out


def snf_step(mats, skip, J, V, reg_diag, out=None, validated=False):
    """One doSimilarityFusionWs cross-diffusion step for matrix `skip`
    (similarity_fusion.py:163-174): S . mean_{m != skip}(mats[m]) . S^T + reg_diag * I.
    mats: list of (n, n) float64 device tensors; J (n, K) column indices, V (n, K) float64
    row-normalised kNN weights of S. Returns a new (n, n) float64 device tensor (or `out`).
    validated=True: J (a device int32 tensor) was checked by `check_knn` already (the fusion loop
    checks each S once, not once per step), so neither the host nor the library checks it again."""
    torch = _torch()
    lib = load_library()
    n = int(mats[0].shape[0])
    for m in mats:
        if m.dtype != torch.float64 or not m.is_cuda or tuple(m.shape) != (n, n) or not m.is_contiguous():
            raise ValueError("snf_step: every matrix must be a contiguous (n, n) float64 device tensor")
    if len(mats) < 2:
        raise ValueError("snf_step: needs at least two matrices (the step averages the others)")
    Jd = _dev(J, torch.int32).contiguous()
    Vd = _dev(V, torch.float64).contiguous()
    if Jd.shape != Vd.shape or Jd.dim() != 2 or Jd.shape[0] != n:
        raise ValueError("snf_step: J and V must both be (n, K)")
    if not validated:
        _check_knn(Jd, n)
    if out is None:
        out = torch.empty((n, n), dtype=torch.float64, device=mats[0].device)
    ptrs = (ctypes.c_void_p * len(mats))(*[m.data_ptr() for m in mats])
    rc = lib.acoss_snf_step(ptrs, len(mats), int(skip), n, _ptr(Jd), _ptr(Vd), int(Jd.shape[1]), float(reg_diag),
                            _ptr(out), 0 if validated else 1, _stream())
    _check(rc, "acoss_snf_step")
    return out


def _knn_dev(J, V, n, validated, what):
    torch = _torch()
    Jd = _dev(J, torch.int32).contiguous()
    Vd = _dev(V, torch.float64).contiguous()
    if Jd.shape != Vd.shape or Jd.dim() != 2 or Jd.shape[0] != n:
        raise ValueError("%s: J and V must both be (n, K)" % what)
    if not validated:
        _check_knn(Jd, n)
    return Jd, Vd


def snf_diffuse_rows(stripes, skip, n, J, V, out=None, validated=False):
    """First half of a row-sharded snf_step (acoss_snf_diffuse_rows): the rows of B = A . S^T
    that belong to this rank's stripe, from the (rows, n) stripes of every matrix. The caller
    all-gathers B's stripes and finishes with snf_left_rows."""
    torch = _torch()
    lib = load_library()
    rows = int(stripes[0].shape[0]) if stripes else 0
    for m in stripes:
        if m.dtype != torch.float64 or not m.is_cuda or tuple(m.shape) != (rows, n) or not m.is_contiguous():
            raise ValueError("snf_diffuse_rows: every stripe must be a contiguous (rows, n) float64 device tensor")
    if len(stripes) < 2:
        raise ValueError("snf_diffuse_rows: needs at least two matrices (the step averages the others)")
    Jd, Vd = _knn_dev(J, V, n, validated, "snf_diffuse_rows")
    if out is None:
        out = torch.empty((rows, n), dtype=torch.float64, device=stripes[0].device)
    ptrs = (ctypes.c_void_p * len(stripes))(*[m.data_ptr() for m in stripes])
    rc = lib.acoss_snf_diffuse_rows(ptrs, len(stripes), int(skip), int(n), rows, _ptr(Jd), _ptr(Vd), int(Jd.shape[1]),
                                    _ptr(out), 0 if validated else 1, _stream())
    _check(rc, "acoss_snf_diffuse_rows")
    return out


def snf_left_rows(B, row0, rows, J, V, reg_diag, out=None, validated=False):
    """Second half of a row-sharded snf_step (acoss_snf_left_rows): rows [row0, row0 + rows) of
    S . B + reg_diag * I from the whole (n, n) B."""
    torch = _torch()
    lib = load_library()
    n = int(B.shape[0])
    if B.dtype != torch.float64 or not B.is_cuda or tuple(B.shape) != (n, n) or not B.is_contiguous():
        raise ValueError("snf_left_rows: B must be a contiguous (n, n) float64 device tensor")
    Jd, Vd = _knn_dev(J, V, n, validated, "snf_left_rows")
    if out is None:
        out = torch.empty((rows, n), dtype=torch.float64, device=B.device)
    rc = lib.acoss_snf_left_rows(_ptr(B), n, int(row0), int(rows), _ptr(Jd), _ptr(Vd), int(Jd.shape[1]),
                                 float(reg_diag), _ptr(out), 0 if validated else 1, _stream())
    _check(rc, "acoss_snf_left_rows")
    return out


def simple_mp_packed(flat, track_off, track_len, pairs, sslen=10, apply_oti=True):
    """SiMPle over packed (12 x n_t) float64 blocks: flat device buffer, element offsets,
    lengths (columns). Returns (score f64 (P,), oti i32 (P,)) device tensors."""
    torch = _torch()
    lib = load_library()
    lens = np.asarray(track_len.cpu() if isinstance(track_len, torch.Tensor) else track_len, np.int64)
    pairs, _ = _pairs_dev(pairs, len(lens))
    P = pairs.shape[0]
    score = torch.empty(P, dtype=torch.float64, device="cuda")
    oti = torch.empty(P, dtype=torch.int32, device="cuda")
    # keep every device buffer referenced until the launch is queued: a temporary passed as
    # _ptr(_dev(...)) returns to torch's caching allocator at once and can be reused
    flat_d = _dev(flat, torch.float64)
    off_d = _dev(track_off, torch.int64)
    len_d = _dev(lens.astype(np.int32), torch.int32)
    rc = lib.acoss_simple_mp(_ptr(flat_d), _ptr(off_d), _ptr(len_d), len(lens), int(lens.max(initial=0)),
                             _ptr(pairs), int(P), int(sslen), int(bool(apply_oti)), _ptr(score), _ptr(oti), _stream())
    _check(rc, "acoss_simple_mp")
    return score, oti


def simple_mp(feats, pairs, sslen=10, apply_oti=True):
    """SiMPle median matrix-profile distance (simple_silva.py:45-118) of ordered pairs.
    feats: list of (12, n) float64 arrays; pairs (P, 2) (query, reference).
    Returns (score f64 (P,), oti i32 (P,)) device tensors; the reference stores -score."""
    torch = _torch()
    mats = [np.asarray(f) if not isinstance(f, torch.Tensor) else f for f in feats]
    for f in mats:
        if f.shape[0] != 12:
            raise ValueError("SiMPle features are (12, n) blocks")
    flat, off, _, cols, _, _ = _pack_mats(mats, torch.float64)
    return simple_mp_packed(flat, off, cols, pairs, sslen, apply_oti)


def simple_profile_offsets(track_len, pairs, sslen):
    """Where each pair's matrix profile starts in the ragged output of simple_profile (host only,
    pure numpy): int64 (P + 1,), pair p's rows at [off[p], off[p + 1]), as many as its query has
    length-sslen subsequences, max(len[query] - sslen + 1, 0)."""
    lens = np.asarray(track_len, np.int64).reshape(-1)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(pairs) and (int(pairs.min()) < 0 or int(pairs.max()) >= len(lens)):
        raise ValueError("pair indices must lie in [0, %d)" % len(lens))
    off = np.zeros(len(pairs) + 1, np.int64)
    np.cumsum(np.maximum(lens[pairs[:, 0]] - int(sslen) + 1, 0), out=off[1:])
    return off


def simple_profile_packed(flat, track_off, track_len, pairs, sslen=10, apply_oti=True):
    """The SiMPle matrix profile and its index per ordered pair (acoss_simple_profile) over packed
    (12 x n_t) float64 blocks, as simple_mp_packed takes them. Returns a dict of device tensors:
    off i64 (P + 1,) (simple_profile_offsets), mp f64 and mpi i32 (off[-1],) ragged by off (row i
    of pair p: its distance to the nearest reference subsequence and that subsequence's index; NaN
    and -1 where a row has none), score f64 (P,) = median(mp) = simple_mp's, oti i32 (P,)."""
    torch = _torch()
    lib = load_library()
    lens = np.asarray(track_len.cpu() if isinstance(track_len, torch.Tensor) else track_len, np.int64)
    pairs, host_pairs = _pairs_dev(pairs, len(lens))
    if host_pairs is None:
        host_pairs = pairs.cpu().numpy()
    P = pairs.shape[0]
    off = simple_profile_offsets(lens, host_pairs, sslen)
    total = int(off[-1])
    mp = torch.empty(total, dtype=torch.float64, device="cuda")
    mpi = torch.empty(total, dtype=torch.int32, device="cuda")
    score = torch.empty(P, dtype=torch.float64, device="cuda")
    oti = torch.empty(P, dtype=torch.int32, device="cuda")
    flat_d = _dev(flat, torch.float64)
    off_d = _dev(track_off, torch.int64)
    len_d = _dev(lens.astype(np.int32), torch.int32)
    poff_d = _dev(off, torch.int64)
    rc = lib.acoss_simple_profile(_ptr(flat_d), _ptr(off_d), _ptr(len_d), len(lens), int(lens.max(initial=0)),
                                  _ptr(pairs), int(P), int(sslen), int(bool(apply_oti)), _ptr(poff_d), total,
                                  _ptr(mp), _ptr(mpi), _ptr(score), _ptr(oti), _stream())
    _check(rc, "acoss_simple_profile")
    return {"off": poff_d, "mp": mp, "mpi": mpi, "score": score, "oti": oti}


def simple_profile(feats, pairs, sslen=10, apply_oti=True):
    """simple_profile_packed for a list of (12, n) float64 arrays, as simple_mp takes them."""
    torch = _torch()
    mats = [np.asarray(f) if not isinstance(f, torch.Tensor) else f for f in feats]
    for f in mats:
        if f.shape[0] != 12:
            raise ValueError("SiMPle features are (12, n) blocks")
    flat, off, _, cols, _, _ = _pack_mats(mats, torch.float64)
    return simple_profile_packed(flat, off, cols, pairs, sslen, apply_oti)


def _self_excl(sslen, excl):
    """The exclusion half-width of a self-join: sslen // 2 unless given; never negative."""
    excl = int(sslen) // 2 if excl is None else int(excl)
    if excl < 0:
        raise ValueError("excl must be >= 0, got %d" % excl)
    return excl


def simple_self_profile_offsets(track_len, tracks, sslen):
    """Where each listed track's self-profile starts in the ragged output of simple_self_profile
    (host only, pure numpy): int64 (n_sel + 1,), entry e's rows at [off[e], off[e + 1]), as many as
    the track has length-sslen subsequences, max(len[tracks[e]] - sslen + 1, 0)."""
    lens = np.asarray(track_len, np.int64).reshape(-1)
    tracks = np.asarray(tracks, np.int64).reshape(-1)
    if len(tracks) and (int(tracks.min()) < 0 or int(tracks.max()) >= len(lens)):
        raise ValueError("track indices must lie in [0, %d)" % len(lens))
    off = np.zeros(len(tracks) + 1, np.int64)
    np.cumsum(np.maximum(lens[tracks] - int(sslen) + 1, 0), out=off[1:])
    return off


def simple_self_profile_packed(flat, track_off, track_len, tracks, sslen=10, excl=None):
    """The SiMPle self-join per listed track (acoss_simple_self_profile) over packed (12 x n_t)
    float64 blocks, as simple_mp_packed takes them: the matrix profile of a track against itself
    without the matches within excl subsequences of the row itself (excl=None: sslen // 2).
    Returns a dict of device tensors: off i64 (n_sel + 1,) (simple_self_profile_offsets), mp f64
    and mpi i32 (off[-1],) ragged by off (row i of entry e: its distance to the nearest admissible
    subsequence of the same track and that subsequence's index; NaN and -1 where there is none),
    motif i32 (n_sel, 2) (the row of the smallest mp and its mpi: the repeated section) and discord
    i32 (n_sel,) (the row of the largest mp); -1 for a track without a row that is not NaN."""
    excl = _self_excl(sslen, excl)
    torch = _torch()
    lib = load_library()
    lens = np.asarray(track_len.cpu() if isinstance(track_len, torch.Tensor) else track_len, np.int64)
    host_tracks = np.asarray(tracks.cpu() if isinstance(tracks, torch.Tensor) else tracks, np.int64).reshape(-1)
    off = simple_self_profile_offsets(lens, host_tracks, sslen)
    n_sel, total = len(host_tracks), int(off[-1])
    mp = torch.empty(total, dtype=torch.float64, device="cuda")
    mpi = torch.empty(total, dtype=torch.int32, device="cuda")
    motif = torch.empty((n_sel, 2), dtype=torch.int32, device="cuda")
    discord = torch.empty(n_sel, dtype=torch.int32, device="cuda")
    flat_d = _dev(flat, torch.float64)
    off_d = _dev(track_off, torch.int64)
    len_d = _dev(lens.astype(np.int32), torch.int32)
    trk_d = _dev(host_tracks.astype(np.int32), torch.int32)
    poff_d = _dev(off, torch.int64)
    rc = lib.acoss_simple_self_profile(_ptr(flat_d), _ptr(off_d), _ptr(len_d), len(lens), int(lens.max(initial=0)),
                                       _ptr(trk_d), n_sel, int(sslen), excl, _ptr(poff_d), total, _ptr(mp), _ptr(mpi),
                                       _ptr(motif), _ptr(discord), _stream())
    _check(rc, "acoss_simple_self_profile")
    return {"off": poff_d, "mp": mp, "mpi": mpi, "motif": motif, "discord": discord}


def simple_self_profile(feats, tracks=None, sslen=10, excl=None):
    """simple_self_profile_packed for a list of (12, n) float64 arrays, as simple_mp takes them;
    tracks=None profiles every one of them."""
    excl = _self_excl(sslen, excl)
    torch = _torch()
    mats = [np.asarray(f) if not isinstance(f, torch.Tensor) else f for f in feats]
    for f in mats:
        if f.shape[0] != 12:
            raise ValueError("SiMPle features are (12, n) blocks")
    flat, off, _, cols, _, _ = _pack_mats(mats, torch.float64)
    if tracks is None:
        tracks = np.arange(len(mats), dtype=np.int32)
    return simple_self_profile_packed(flat, off, cols, tracks, sslen, excl)


def median_downsample(feats, track_off, track_len, factor=40):
    """librosa.util.sync(chroma.T, arange(0, n, factor), aggregate=np.median).T per track
    (rqa_serra09.py:44-53). Returns (out (sum ceil(n/f), 12) f32 device, out_off i64, out_len i32)."""
    torch = _torch()
    lib = load_library()
    lens = np.asarray(track_len.cpu() if isinstance(track_len, torch.Tensor) else track_len, np.int64)
    out_len = (lens + factor - 1) // factor
    out_off = np.zeros(len(lens), np.int64)
    if len(lens) > 1:
        out_off[1:] = np.cumsum(out_len[:-1])
    out = torch.empty((max(1, int(out_len.sum())), 12), dtype=torch.float32, device="cuda")
    f = _dev(feats, torch.float32)
    o = _dev(track_off, torch.int64)
    ln = _dev(lens.astype(np.int32), torch.int32)
    oo = _dev(out_off, torch.int64)
    rc = lib.acoss_median_downsample(_ptr(f), _ptr(o), _ptr(ln), len(lens), int(lens.max(initial=0)), int(factor),
                                     _ptr(out), _ptr(oo), _stream())
    _check(rc, "acoss_median_downsample")
    return out[: int(out_len.sum())], out_off, out_len.astype(np.int32)


def hann_smoothing(win_len_smooth=4):
    """Simple.smooth's window: scipy/librosa get_window('hann', L + 2, fftbins=False), sum 1."""
    from scipy import signal
    w = signal.get_window("hann", win_len_smooth + 2, fftbins=False)
    return np.ascontiguousarray(w / np.sum(w), np.float64)


def simple_features(feats, track_off, track_len, win=200, skip=100, win_len_smooth=4):
    """Simple.load_features for every track (simple_silva.py:34-43,56-66).
    Returns (out flat f64 device, out_off i64 (element offsets), T i32 (columns per track));
    track t is out[out_off[t]: out_off[t] + 12*T[t]].view(12, T[t])."""
    torch = _torch()
    lib = load_library()
    lens = np.asarray(track_len.cpu() if isinstance(track_len, torch.Tensor) else track_len, np.int64)
    T = lens // skip
    out_off = np.zeros(len(lens), np.int64)
    if len(lens) > 1:
        out_off[1:] = np.cumsum(12 * T[:-1])
    total = int(12 * T.sum())
    out = torch.empty(max(1, total), dtype=torch.float64, device="cuda")
    w = hann_smoothing(win_len_smooth)
    f = _dev(feats, torch.float32)
    o = _dev(track_off, torch.int64)
    ln = _dev(lens.astype(np.int32), torch.int32)
    oo = _dev(out_off, torch.int64)
    rc = lib.acoss_simple_features(_ptr(f), _ptr(o), _ptr(ln), len(lens), int(win), int(skip),
                                   w.ctypes.data_as(ctypes.c_void_p), len(w), _ptr(out), _ptr(oo), total, _stream())
    _check(rc, "acoss_simple_features")
    return out[:total], out_off, T.astype(np.int32)


def check_ef_binarize(mutual):
    """The `mutual` flag every EarlyFusion layer takes (a bool; include/acoss_hip.h, "mutual") ->
    ACOSS_EF_BIN_ROWS or ACOSS_EF_BIN_MUTUAL; ValueError for anything but a bool."""
    if not isinstance(mutual, (bool, np.bool_)):
        raise ValueError("mutual must be True or False, not %r" % (mutual,))
    return EF_BINARIZE["mutual" if mutual else "rows"]


def ef_mutual_suffix(mutual=False):
    """What a cache or result name carries for the binarisation: '' for the row rule, '-mutual'."""
    return "-mutual" if check_ef_binarize(mutual) else ""


def ef_neighbour_error(nb_query, nb_ref, kappa, K, mutual=False):
    """The ValueError the reference raises for a pair of block counts, or None (host-only, no GPU).
    csm_to_binary takes argpartition(D, nn, 1) with nn = round(kappa * ncols) (kappa < 1) or kappa,
    which raises unless nn < ncols (cross_recurrence.py:150-156); getWCSM takes np.partition(CSM, K)
    along the columns and the rows, which raises unless K < ncols and K < nrows
    (similarity_fusion.py:47-50). nb_query / nb_ref: block counts (arrays) of each pair's songs.
    mutual: the column half takes the same count of the query's blocks (CSMToBinary(D.T) in Tralie's
    CSMToBinaryMutual), so the same error for round(kappa * nrows) >= nrows."""
    check_ef_binarize(mutual)
    nq = np.asarray(nb_query, np.int64)
    nr = np.asarray(nb_ref, np.int64)
    if kappa != 0:
        for n in (nr, nq) if mutual else (nr,):
            nn = np.round(kappa * n).astype(np.int64) if kappa < 1 else np.full(n.shape, int(kappa), np.int64)
            bad = np.flatnonzero(nn >= n)
            if len(bad):
                b = bad[0]
                return ValueError("kth(=%d) out of bounds (%d)" % (nn[b], n[b]))
    bad = np.flatnonzero((K >= nr) | (K >= nq))
    if len(bad):
        b = bad[0]
        return ValueError("kth(=%d) out of bounds (%d)" % (K, min(nr[b], nq[b])))
    return None


def _check_ef_neighbours(bank, pairs, kappa, K, mutual=False):
    """Reject pairs whose block counts the reference's argpartition / partition would refuse (see
    ef_neighbour_error) before the kernels run. The smallest counts decide: both conditions are
    monotone in the block count (n - round(kappa n) never decreases with n for kappa < 1)."""
    if isinstance(pairs, np.ndarray):  # host pairs and the bank's host block counts: no sync
        nbp = np.asarray(bank["nb_host"])[pairs]
    else:
        nbp = bank["nb"].long()[pairs.long()]
    lo_q, lo_r = int(nbp[:, 0].min()), int(nbp[:, 1].min())
    err = ef_neighbour_error([lo_q], [lo_r], kappa, K, mutual)
    if err is not None:
        raise err


def _ef_band_order(pairs, T):
    """The order acoss_earlyfusion and its locate / path forms run a large pair list in (a permutation of
    range(P), device int64), or None for 4096 pairs or fewer.
    Pairs in (reference band, query) order: a band of 16 reference tracks' block rows stays
    cache-resident while every query track's rows stream past it once per band (an i-major
    pair list streams every reference track's rows once per query). Results go back to the
    caller's order. Da-TACOS shape, 15,000 songs: 3.29M -> 4.07M pairs/s (bands of 16..128
    alike; profiles/r05/ef_short/efband15k_*.log). The runs holding the whole band come
    first, so they start at multiples of 16 and the CSM kernel's groups of 64 pairs hold
    four queries with the same 16 references (k_ef_csm_pack packs their rows and columns;
    profiles/r06/ef_pack/README.txt). No host synchronisation: run lengths by scatter_add."""
    torch = _torch()
    P = pairs.shape[0]
    if P <= 4096:
        return None
    band = 16
    key = (pairs[:, 1].to(torch.int64) // band) * T + pairs[:, 0].to(torch.int64)
    order = torch.argsort(key, stable=True)
    ks = key[order]
    start = torch.ones(P, dtype=torch.bool, device=ks.device)
    start[1:] = ks[1:] != ks[:-1]
    rid = torch.cumsum(start, 0) - 1
    runlen = torch.zeros(P, dtype=torch.int64, device=ks.device).scatter_add_(0, rid, torch.ones_like(rid))[rid]
    return order[torch.argsort((runlen < band).to(torch.int8), stable=True)]


def earlyfusion(bank, pairs, kappa=0.1, K=10, mu=0.5, mutual=False):
    """Batched EarlyFusion scores (earlyfusion_traile.py:157-198). bank: dict of device tensors
    'mfccs', 'ssms', 'chromas' (sum nb x d, float32), 'chroma_med' (T x 12), 'off' (T,) int64,
    'nb' (T,) int32 and host 'max_blocks'. Returns (P, 4) float64 device tensor with columns
    mfccs, ssms, chromas, early. mutual: binarise by mutual nearest neighbours (acoss_earlyfusion2
    with ACOSS_EF_BIN_MUTUAL; include/acoss_hip.h) instead of the reference's row rule."""
    binarize = check_ef_binarize(mutual)
    torch = _torch()
    lib = load_library()
    pairs, host = _pairs_dev(pairs, int(bank["nb"].shape[0]))
    P = pairs.shape[0]
    out = torch.empty((P, 4), dtype=torch.float64, device="cuda")
    if P == 0:
        return out
    _check_ef_neighbours(bank, pairs if host is None or "nb_host" not in bank else host, kappa, K, mutual)
    T = int(bank["nb"].shape[0])
    order = _ef_band_order(pairs, T)
    if order is not None:
        pairs = pairs[order].contiguous()
    dst = out if order is None else torch.empty_like(out)
    lead = (_ptr(bank["mfccs"]), _ptr(bank["ssms"]), _ptr(bank["chromas"]), _ptr(bank["chroma_med"]),
            _ptr(bank["off"]), _ptr(bank["nb"]), T, int(bank["max_blocks"]),
            int(bank["mfccs"].shape[1]), int(bank["ssms"].shape[1]), int(bank["chromas"].shape[1]),
            _ptr(pairs), int(P), float(kappa), int(K), float(mu))
    if mutual:
        rc = lib.acoss_earlyfusion2(*lead, binarize, _ptr(dst), _stream())
    else:
        rc = lib.acoss_earlyfusion(*lead, _ptr(dst), _stream())
    _check(rc, "acoss_earlyfusion2" if mutual else "acoss_earlyfusion")
    if order is not None:
        out[order] = dst
    return out


EF_SNF_MAX_K = 64         # neighbours per row of acoss_earlyfusion_snf
EF_SNF_MAX_BLOCKS = 512   # blocks per track
EF_SNF_LDS_N = 101        # pairs of up to this many blocks in all fuse inside one workgroup's LDS


def ef_snf_pair_ok(M, N, K):
    """Whether the reference can fuse a pair of M and N blocks at all (host only, numpy): getW's
    np.partition(DSym, k + 1) needs 1 <= k1 <= M - 2 and 1 <= k2 <= N - 2 (k = 0 divides by zero),
    getS's argpartition K < M + N; k1 = int(K M / (M + N)), k2 = K - k1 (similarity_fusion.py:93-94)."""
    M = np.asarray(M, np.int64)
    N = np.asarray(N, np.int64)
    k1 = (K * M.astype(np.float64) / np.maximum(M + N, 1)).astype(np.int64)
    k2 = K - k1
    return (M + N > K) & (k1 >= 1) & (k1 <= M - 2) & (k2 >= 1) & (k2 <= N - 2)


def ef_snf_cross_offsets(nb, pairs):
    """Where each pair's M x N cross matrix starts in the ragged output of earlyfusion_snf (host
    only): int64 (P + 1,)."""
    nb = np.asarray(nb, np.int64).reshape(-1)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(pairs) and (int(pairs.min()) < 0 or int(pairs.max()) >= len(nb)):
        raise ValueError("pair indices must lie in [0, %d)" % len(nb))
    off = np.zeros(len(pairs) + 1, np.int64)
    np.cumsum(nb[pairs[:, 0]] * nb[pairs[:, 1]], out=off[1:])
    return off


def ef_snf_check_args(kappa, K, niters, reg_diag, max_blocks=None):
    """The argument errors of earlyfusion_snf that need no GPU (ValueError). K is held to [1, 64]
    whatever max_blocks is: each pair answers for it on its own (ef_snf_pair_ok)."""
    if int(niters) != niters or niters < 0:
        raise ValueError("niters must be a non-negative integer, got %r" % (niters,))
    if not reg_diag >= 0:
        raise ValueError("reg_diag must be >= 0, got %r" % (reg_diag,))
    if int(K) != K or not 1 <= K <= EF_SNF_MAX_K:
        raise ValueError("K must be an integer in [1, %d], got %r" % (EF_SNF_MAX_K, K))
    if not kappa >= 0:
        raise ValueError("kappa must be >= 0, got %r" % (kappa,))
    if max_blocks is not None and max_blocks > EF_SNF_MAX_BLOCKS:
        raise ValueError("early SNF takes tracks of at most %d blocks, got %d" % (EF_SNF_MAX_BLOCKS, max_blocks))


def earlyfusion_snf(bank, pairs, kappa, K, niters, reg_diag=1.0, want_cross=False, mu=0.5, mutual=False,
                    want_binary=False):
    """The per-pair similarity network fusion score of EarlyFusion (acoss_earlyfusion_snf; the
    definition is in include/acoss_hip.h). bank as earlyfusion() takes it. Returns a dict of device
    tensors: "score" f64 (P,), NaN for a pair the reference cannot fuse (ef_snf_pair_ok); with
    want_cross also "cross_off" i64 (P + 1,) and "cross" f64 (cross_off[-1],), pair p's M x N
    cross block of the fused matrix, row-major (both None otherwise). A kappa whose neighbour count
    reaches a reference's block count raises the reference's ValueError, as earlyfusion() does.
    mutual: the binary matrix keeps a cell only if it is also among the largest of its column
    (acoss_earlyfusion_snf2; under it the same ValueError for a query's block count). want_binary:
    also "binary" u8 (cross_off[-1],), pair p's M x N binary matrix as Smith-Waterman read it, at
    cross_off[p] (all zero for a pair that cannot be fused), and "cross_off"."""
    binarize = check_ef_binarize(mutual)
    ef_snf_check_args(kappa, K, niters, reg_diag, bank.get("max_blocks"))
    torch = _torch()
    lib = load_library()
    T = int(bank["nb"].shape[0])
    pairs, host = _pairs_dev(pairs, T)
    P = pairs.shape[0]
    score = torch.empty(P, dtype=torch.float64, device="cuda")
    nb_host = np.asarray(bank["nb_host"]) if "nb_host" in bank else bank["nb"].cpu().numpy()
    if host is None:
        host = pairs.cpu().numpy()
    if P and kappa != 0:  # csm_to_binary's argpartition(D, nn, 1) needs nn < ncols (cross_recurrence.py:150-156)
        lo = int(nb_host[host[:, 1]].min())  # n - round(kappa n) never decreases with n: the smallest decides
        nn = int(np.round(kappa * lo)) if kappa < 1 else int(kappa)
        if nn >= lo:
            raise ValueError("kth(=%d) out of bounds (%d)" % (nn, lo))
        if mutual:
            err = ef_neighbour_error([int(nb_host[host[:, 0]].min())], [lo], kappa, 0, True)
            if err is not None:
                raise err
    off_d = cross = binary = None
    total = 0
    if want_cross or want_binary:
        off = ef_snf_cross_offsets(nb_host, host)
        total = int(off[-1])
        off_d = _dev(off, torch.int64)
        if want_cross:
            cross = torch.empty(total, dtype=torch.float64, device="cuda")
        if want_binary:
            binary = torch.zeros(total, dtype=torch.uint8, device="cuda")
    if P:
        lead = (_ptr(bank["mfccs"]), _ptr(bank["ssms"]), _ptr(bank["chromas"]), _ptr(bank["chroma_med"]),
                _ptr(bank["off"]), _ptr(bank["nb"]), T, int(bank["max_blocks"]), int(bank["mfccs"].shape[1]),
                int(bank["ssms"].shape[1]), int(bank["chromas"].shape[1]), _ptr(pairs), int(P), float(kappa), int(K),
                float(mu))
        tail = (int(niters), float(reg_diag), _ptr(score), _ptr(off_d), total,
                _ptr(cross) if total and want_cross else None)
        if mutual or want_binary:
            rc = lib.acoss_earlyfusion_snf2(*lead, binarize, *tail, _ptr(binary) if total and want_binary else None,
                                            _stream())
        else:
            rc = lib.acoss_earlyfusion_snf(*lead, *tail, _stream())
        _check(rc, "acoss_earlyfusion_snf2" if mutual or want_binary else "acoss_earlyfusion_snf")
    return {"score": score, "cross_off": off_d, "cross": cross, "binary": binary}


def _ef_args(bank, pairs, kappa, K, mu, mutual=False):
    """The arguments acoss_earlyfusion and its locate / path forms share, after earlyfusion()'s checks:
    (device pairs (P, 2) in the order they run in, that order (_ef_band_order) or None, the leading
    arguments up to the feature widths, the trailing kappa, K, mu)."""
    pairs, host = _pairs_dev(pairs, int(bank["nb"].shape[0]))
    if pairs.shape[0]:
        _check_ef_neighbours(bank, pairs if host is None or "nb_host" not in bank else host, kappa, K, mutual)
    order = _ef_band_order(pairs, int(bank["nb"].shape[0]))
    if order is not None:
        pairs = pairs[order].contiguous()
    lead = (_ptr(bank["mfccs"]), _ptr(bank["ssms"]), _ptr(bank["chromas"]), _ptr(bank["chroma_med"]),
            _ptr(bank["off"]), _ptr(bank["nb"]), int(bank["nb"].shape[0]), int(bank["max_blocks"]),
            int(bank["mfccs"].shape[1]), int(bank["ssms"].shape[1]), int(bank["chromas"].shape[1]))
    return pairs, order, lead, (float(kappa), int(K), float(mu))


def _unorder(order, t):
    """A per-pair result of pairs run in `order` (None: as given), back in the caller's order."""
    if order is None:
        return t
    out = t.new_empty(t.shape)
    out[order] = t
    return out


def earlyfusion_locate(bank, pairs, kappa=0.1, K=10, mu=0.5, mutual=False):
    """earlyfusion() with where each of the four alignments lies (acoss_earlyfusion_locate): device
    tensors {"scores" (P, 4) f64, earlyfusion()'s bit for bit, "seg" (P, 4, 4) i32}: seg[p, s] =
    (r0, c0, r1, c1), the first and last cell of the alignment in matrix s (mfccs, ssms, chromas,
    early) of pair p, rows the query's blocks and columns the reference's, (-1, -1, -1, -1) where
    the score is 0. mutual: as earlyfusion() (acoss_earlyfusion_locate2)."""
    binarize = check_ef_binarize(mutual)
    pairs, order, lead, tail = _ef_args(bank, pairs, kappa, K, mu, mutual)
    P = pairs.shape[0]
    scores, seg = _empty("float64", P, 4), _empty("int32", P, 4, 4)
    if P and mutual:
        rc = load_library().acoss_earlyfusion_locate2(*lead, _ptr(pairs), int(P), *tail, binarize, _ptr(scores),
                                                      _ptr(seg), _stream())
        _check(rc, "acoss_earlyfusion_locate2")
    elif P:
        rc = load_library().acoss_earlyfusion_locate(*lead, _ptr(pairs), int(P), *tail, _ptr(scores), _ptr(seg),
                                                     _stream())
        _check(rc, "acoss_earlyfusion_locate")
    return {"scores": _unorder(order, scores), "seg": _unorder(order, seg)}


def earlyfusion_path(bank, pairs, kappa=0.1, K=10, mu=0.5, mutual=False):
    """earlyfusion_locate with the four whole paths of every pair (acoss_earlyfusion_path): {"scores",
    "seg", "path_off" (4 P + 1,) i64, "cells" (total, 2) i32}; the path of matrix s of pair p is
    cells[path_off[4 p + s]:path_off[4 p + s + 1]], (query block, reference block) cells in steps
    (1, 1), (2, 1), (1, 2). The pairs go to the library in chunks whose padded output stays near
    PATH_CHUNK_BYTES; each is compacted on the device. mutual: as earlyfusion() (acoss_earlyfusion_path2)."""
    binarize = check_ef_binarize(mutual)
    torch = _torch()
    lib = load_library()
    pairs, order, lead, tail = _ef_args(bank, pairs, kappa, K, mu, mutual)
    P = pairs.shape[0]
    scores, seg, lens = _empty("float64", P, 4), _empty("int32", P, 4, 4), _empty("int32", P, 4)
    cap = max(1, sw_path_bound(int(bank["max_blocks"]), int(bank["max_blocks"])))
    chunk = max(1, PATH_CHUNK_BYTES // (4 * 8 * cap))
    parts = []
    for a in range(0, P, chunk):
        n = min(chunk, P - a)
        padded = torch.empty((4 * n, cap, 2), dtype=torch.int32, device="cuda")
        out_args = (_ptr(scores[a:a + n]), _ptr(seg[a:a + n]), int(cap), _ptr(lens[a:a + n]), _ptr(padded), _stream())
        if mutual:
            rc = lib.acoss_earlyfusion_path2(*lead, _ptr(pairs[a:a + n]), int(n), *tail, binarize, *out_args)
        else:
            rc = lib.acoss_earlyfusion_path(*lead, _ptr(pairs[a:a + n]), int(n), *tail, *out_args)
        _check(rc, "acoss_earlyfusion_path2" if mutual else "acoss_earlyfusion_path")
        parts.append(_compact_paths(lens[a:a + n].reshape(-1), padded)[1])
    cells = torch.cat(parts) if parts else torch.empty((0, 2), dtype=torch.int32, device="cuda")
    run_off = torch.zeros(4 * P + 1, dtype=torch.int64, device="cuda")  # in the order the pairs ran in
    run_off[1:] = torch.cumsum(lens.reshape(-1).to(torch.int64), 0)
    if order is None:
        return {"scores": scores, "seg": seg, "path_off": run_off, "cells": cells}
    # back to the caller's order: every cell moves by the shift of its matrix' first cell
    lens_o = _unorder(order, lens).reshape(-1).to(torch.int64)
    path_off = torch.zeros(4 * P + 1, dtype=torch.int64, device="cuda")
    path_off[1:] = torch.cumsum(lens_o, 0)
    mat_o = (4 * order[:, None] + torch.arange(4, device="cuda")[None, :]).reshape(-1)  # caller's index of run matrix k
    shift = torch.repeat_interleave(path_off[:-1][mat_o] - run_off[:-1], lens.reshape(-1).to(torch.int64))
    out = torch.empty_like(cells)
    out[torch.arange(cells.shape[0], device="cuda") + shift] = cells
    return {"scores": _unorder(order, scores), "seg": _unorder(order, seg), "path_off": path_off, "cells": out}


def ef_block_features(chromas, mfccs, onsets, blocksize=20, mfccs_per_block=50, chromas_per_block=40):
    """EarlyFusion block features of a batch of tracks on the device (acoss_ef_block_features).
    chromas: list of (n_t, 12); mfccs: list of (m_t, d) frame-major (mfcc_htk.T; m_t may differ from
    n_t: the extractor's MFCC frames are longer, features.py:884); onsets: list of frame-index arrays.
    Block b spans mfcc[o[b]:o[b+blocksize-1]] and chroma[o[b]:o[b+blocksize]], each clamped to its
    own length as the reference's slicing (resize_block, earlyfusion_traile.py:240); an empty span
    raises ValueError, as the reference's resize does. NaN MFCCs become 0 (:98). Returns a dict of
    device tensors 'mfccs' (B, R*d), 'ssms' (B, R(R-1)/2), 'chromas' (B, Rc*12), 'chroma_med'
    (T, 12) and host 'block_off' (T,) int64 / 'n_blocks' (T,) int32 (blocks of track t: rows
    block_off[t] .. + n_blocks[t])."""
    torch = _torch()
    lib = load_library()
    T = len(chromas)
    if not (len(mfccs) == len(onsets) == T):
        raise ValueError("one chroma, mfcc and onset array per track")
    n = np.array([len(c) for c in chromas], np.int64)
    nm = np.array([len(m) for m in mfccs], np.int64)
    d = int(np.asarray(mfccs[0]).shape[1]) if T else 20
    nb = np.zeros(T, np.int64)
    for t in range(T):
        o = np.asarray(onsets[t], np.int64)
        if np.asarray(mfccs[t]).ndim != 2 or np.asarray(mfccs[t]).shape[1] != d:
            raise ValueError("track %d: mfcc must be (n_frames, %d) like the first track's" % (t, d))
        if len(o) < blocksize:  # the reference's np.zeros((n_beats - blocksize, ...)) raises here (:106)
            raise ValueError("track %d: %d beats, fewer than blocksize=%d (negative dimensions are not allowed)"
                             % (t, len(o), blocksize))
        nb[t] = len(o) - blocksize
        if nb[t]:
            if o.min() < 0:
                raise ValueError("track %d: negative onset frame" % t)
            b = np.arange(nb[t])
            # the clamped spans of every block (Python slicing); the reference's resize raises on
            # an empty one (skimage.transform.resize of a (0, d) block)
            m1, m2 = np.minimum(o[b], nm[t]), np.minimum(o[b + blocksize - 1], nm[t])
            c1, c2 = np.minimum(o[b], n[t]), np.minimum(o[b + blocksize], n[t])
            if np.any(m2 <= m1) or np.any(c2 <= c1):
                bad = int(np.flatnonzero((m2 <= m1) | (c2 <= c1))[0])
                raise ValueError("track %d: beat block %d spans no frames (onsets %d..%d, %d chroma / %d mfcc "
                                 "frames)" % (t, bad, o[bad], o[bad + blocksize], n[t], nm[t]))
    foff = np.zeros(T, np.int64)
    foff[1:] = np.cumsum(n[:-1])
    moff = np.zeros(T, np.int64)
    moff[1:] = np.cumsum(nm[:-1])
    ooff = np.zeros(T, np.int64)
    ooff[1:] = np.cumsum([len(o) for o in onsets][:-1])
    boff = np.zeros(T, np.int64)
    boff[1:] = np.cumsum(nb[:-1])
    B = int(nb.sum())
    mf = np.concatenate([np.asarray(m, np.float32) for m in mfccs]) if T else np.zeros((0, d), np.float32)
    mf = np.where(np.isnan(mf), np.float32(0), mf)
    ch = np.concatenate([np.asarray(c, np.float32) for c in chromas]) if T else np.zeros((0, 12), np.float32)
    on = np.concatenate([np.asarray(o, np.int64) for o in onsets]) if T else np.zeros(0, np.int64)
    d_mf, d_ch = _dev(mf, torch.float32), _dev(ch, torch.float32)
    d_foff, d_n = _dev(foff, torch.int64), _dev(n.astype(np.int32), torch.int32)
    d_moff, d_nm = _dev(moff, torch.int64), _dev(nm.astype(np.int32), torch.int32)
    d_on, d_ooff, d_boff = _dev(on, torch.int64), _dev(ooff, torch.int64), _dev(boff, torch.int64)
    R, Rc = int(mfccs_per_block), int(chromas_per_block)
    out = {"mfccs": torch.empty((B, R * d), dtype=torch.float32, device="cuda"),
           "ssms": torch.empty((B, R * (R - 1) // 2), dtype=torch.float32, device="cuda"),
           "chromas": torch.empty((B, Rc * 12), dtype=torch.float32, device="cuda"),
           "chroma_med": torch.empty((T, 12), dtype=torch.float32, device="cuda")}
    rc = lib.acoss_ef_block_features(_ptr(d_mf), _ptr(d_ch), _ptr(d_foff), _ptr(d_n), _ptr(d_moff), _ptr(d_nm),
                                     _ptr(d_on), _ptr(d_ooff), _ptr(d_boff), T, B, int(blocksize), R, Rc, d,
                                     _ptr(out["mfccs"]), _ptr(out["ssms"]), _ptr(out["chromas"]),
                                     _ptr(out["chroma_med"]), _stream())
    _check(rc, "acoss_ef_block_features")
    out["block_off"] = boff
    out["n_blocks"] = nb.astype(np.int32)
    return out


FTM2D_MAX_WINDOWS = 4096  # windows per track (ftm2d.hip sorts them in LDS), as SiMPle caps frames


def ftm2d_bounds(chromas, onsets, win=75):
    """Host half of ftm2d_shingles (no GPU): pack the tracks and build every track's segment
    boundaries, np.unique(concat([0], clip(onsets, 0, n), [n])) (what librosa.util.sync slices at,
    ftm2d.py:58). Raises ValueError naming every track with fewer than `win` beats (the reference's
    btchroma_to_fftmat returns None there and crashes, :129-130) or more than win - 1 + 4096.
    Returns (feats (sum n, 12) f32, off i64, lens i32, bounds i64, bound_off i64 (T + 1))."""
    from .synthetic import pack
    T = len(chromas)
    if len(onsets) != T:
        raise ValueError("one chroma and one onset array per track")
    tracks = [np.asarray(c, np.float32) for c in chromas]
    for t, c in enumerate(tracks):
        if c.ndim != 2 or c.shape[1] != 12:
            raise ValueError("track %d: chroma must be (n_frames, 12)" % t)
    bnds, bad = [], []
    for t, (c, o) in enumerate(zip(tracks, onsets)):
        n = len(c)
        o = np.clip(np.asarray(o, np.int64).ravel(), 0, n)
        b = np.unique(np.concatenate([np.zeros(1, np.int64), o, np.full(1, n, np.int64)]))
        nb = len(b) - 1
        if nb < win:
            bad.append("track %d: %d beats, fewer than WIN=%d" % (t, nb, win))
        elif nb > win - 1 + FTM2D_MAX_WINDOWS:
            bad.append("track %d: %d beats, more than %d (%d windows)" % (t, nb, win - 1 + FTM2D_MAX_WINDOWS,
                                                                        FTM2D_MAX_WINDOWS))
        bnds.append(b)
    if bad:
        raise ValueError("FTM2D: " + "; ".join(bad))
    bound_off = np.zeros(T + 1, np.int64)
    bound_off[1:] = np.cumsum([len(b) for b in bnds])
    bounds = np.concatenate(bnds) if T else np.zeros(0, np.int64)
    feats, off, lens = pack(tracks)
    return feats, off, lens, bounds.astype(np.int64), bound_off


def ftm2d_shingles(chromas, onsets, win=75, pwr=1.96, C=5):
    """FTM2D.load_features for every track (ftm2d.py:52-66): chromas, a list of (n_t, 12) arrays,
    and onsets, a list of frame-index arrays -> (N, 12 * win) float64 device tensor of shingles."""
    packed = ftm2d_bounds(chromas, onsets, win)  # raises before any launch
    torch = _torch()
    lib = load_library()
    feats, off, lens, bounds, bound_off = packed
    T = len(lens)
    out = torch.empty((T, 12 * int(win)), dtype=torch.float64, device="cuda")
    if T == 0:
        return out
    # keep every device buffer referenced until the launch is queued
    f = _dev(feats, torch.float32)
    o = _dev(off, torch.int64)
    ln = _dev(lens, torch.int32)
    b = _dev(bounds, torch.int64)
    bo = _dev(bound_off, torch.int64)
    rc = lib.acoss_ftm2d_shingles(_ptr(f), _ptr(o), _ptr(ln), T, int(lens.max(initial=0)), _ptr(b), _ptr(bo), int(win),
                                  float(pwr), float(C), _ptr(out), _stream())
    _check(rc, "acoss_ftm2d_shingles")
    return out


def ftm2d_beatsync(chromas, onsets, pwr=1.96):
    """The first two steps of ftm2d_shingles alone (parity tests): per track the (12, beats)
    float32 beat-synchronous medians and their float64 chrompwr, as lists of numpy arrays."""
    packed = ftm2d_bounds(chromas, onsets, win=0)
    torch = _torch()
    lib = load_library()
    feats, off, lens, bounds, bound_off = packed
    T = len(lens)
    nb = np.diff(bound_off) - 1
    cols = int(nb.sum())
    sync = torch.empty(max(1, 12 * cols), dtype=torch.float32, device="cuda")
    chroma = torch.empty(max(1, 12 * cols), dtype=torch.float64, device="cuda")
    f = _dev(feats, torch.float32)
    o = _dev(off, torch.int64)
    ln = _dev(lens, torch.int32)
    b = _dev(bounds, torch.int64)
    bo = _dev(bound_off, torch.int64)
    rc = lib.acoss_ftm2d_beatsync(_ptr(f), _ptr(o), _ptr(ln), T, _ptr(b), _ptr(bo), int(nb.max(initial=0)), float(pwr),
                                  _ptr(sync), _ptr(chroma), _stream())
    _check(rc, "acoss_ftm2d_beatsync")
    sh, ch = sync.cpu().numpy(), chroma.cpu().numpy()
    col0 = bound_off[:-1] - np.arange(T)
    return ([sh[12 * c:12 * (c + n)].reshape(12, n) for c, n in zip(col0, nb)],
            [ch[12 * c:12 * (c + n)].reshape(12, n) for c, n in zip(col0, nb)])


def ftm2d_scores(shingles, pairs):
    """FTM2D.similarity (ftm2d.py:85-97): exp(-|s_i - s_j|^2) of the (P, 2) pairs -> (P,) float64
    device tensor. shingles: (N, dim) float64."""
    torch = _torch()
    lib = load_library()
    S = _dev(shingles, torch.float64)
    if S.dim() != 2:
        raise ValueError("shingles must be (N, dim)")
    pairs, _ = _pairs_dev(pairs, int(S.shape[0]))
    P = int(pairs.shape[0])
    out = torch.empty(P, dtype=torch.float64, device="cuda")
    rc = lib.acoss_ftm2d_scores(_ptr(S), int(S.shape[0]), int(S.shape[1]), _ptr(pairs), P, _ptr(out), _stream())
    _check(rc, "acoss_ftm2d_scores")
    return out


FTM2D_MAX_DIM = 1024   # shingle length the pair kernels keep in registers (16 doubles per lane)
FTM2D_MAX_TOPK = 1024  # shortlist length (ftm2d.hip keeps a query's 2k candidates in LDS)


def ftm2d_topk(q, r, k, self_off=-1):
    """The k best references per query without the (n_q, n_r) score matrix (acoss_ftm2d_topk):
    q (n_q, dim) and r (n_r, dim) float64 device tensors -> (idx int32 (n_q, k), score float64
    (n_q, k)) device tensors. Row i lists np.argsort(-scores[i], kind="stable")[:k] and those scores,
    each exactly ftm2d_scores' for the pair; a NaN score is never listed; slots left over hold -1 /
    NaN. self_off >= 0: query i is reference self_off + i, which is left out."""
    torch = _torch()
    lib = load_library()
    for name, t in (("q", q), ("r", r)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.dim() != 2:
            raise ValueError("%s must be a 2-D float64 device tensor" % name)
    if q.shape[1] != r.shape[1]:
        raise ValueError("q and r must have the same row length (%d != %d)" % (q.shape[1], r.shape[1]))
    dim, k, self_off = int(q.shape[1]), int(k), int(self_off)
    if not 1 <= dim <= FTM2D_MAX_DIM:
        raise ValueError("the row length must be in [1, %d], got %d" % (FTM2D_MAX_DIM, dim))
    if not 1 <= k <= FTM2D_MAX_TOPK:
        raise ValueError("k must be in [1, %d], got %d" % (FTM2D_MAX_TOPK, k))
    if self_off < -1:
        raise ValueError("self_off must be -1 (no exclusion) or a reference row, got %d" % self_off)
    q, r = q.contiguous(), r.contiguous()
    n_q, n_r = int(q.shape[0]), int(r.shape[0])
    idx = torch.empty((n_q, k), dtype=torch.int32, device="cuda")
    score = torch.empty((n_q, k), dtype=torch.float64, device="cuda")
    rc = lib.acoss_ftm2d_topk(_ptr(q), n_q, _ptr(r), n_r, dim, self_off, k, _ptr(idx), _ptr(score), _stream())
    _check(rc, "acoss_ftm2d_topk")
    return idx, score


FINISH_MODES = {None: 0, "none": 0, "serra09": 1, "chen": 2}


def ds_finish(D, norm=None, symmetric=True, mode=None, out=None):
    """acoss_ds_finish on a (n, n) float32 device matrix: Ds += Ds.T (symmetric) then the
    Serra09 (D / sqrt(n_j)) or Chen (sqrt(n_j) / D) length normalisation with norm[j] =
    sqrt(n_j) in float64. In place unless `out` is given."""
    torch = _torch()
    lib = load_library()
    if D.dtype != torch.float32 or not D.is_cuda or D.dim() != 2 or D.shape[0] != D.shape[1] or D.stride(1) != 1:
        raise ValueError("ds_finish takes a square float32 CUDA matrix with unit column stride")
    m = FINISH_MODES[mode]
    nrm = _dev(norm, torch.float64) if m else None
    if m and nrm.numel() != D.shape[0]:
        raise ValueError("norm must hold one factor per column")
    out = D if out is None else out
    if out.shape != D.shape or out.dtype != D.dtype or out.stride() != D.stride():
        raise ValueError("out must match D")
    rc = lib.acoss_ds_finish(_ptr(D), int(D.shape[0]), int(D.stride(0)), _ptr(nrm), int(bool(symmetric)), m,
                             _ptr(out), _stream())
    _check(rc, "acoss_ds_finish")
    return out


def eval_ranks(D, pos, q_song, m_off, members):
    """acoss_eval_ranks: rank (1-based) of members[m_off[q]:m_off[q+1]] in row q_song[q] of D,
    in np.argsort(-D', 1, kind='stable') order of the clique-permuted matrix (pos = each song's
    position in that order), diagonal -inf. Returns an int32 numpy array."""
    torch = _torch()
    lib = load_library()
    if D.dtype != torch.float32 or not D.is_cuda or D.stride(1) != 1:
        raise ValueError("eval_ranks takes a float32 CUDA matrix with unit column stride")
    n = int(D.shape[0])
    pos = _dev(pos, torch.int32)
    q_song = _dev(q_song, torch.int32)
    m_off = _dev(m_off, torch.int64)
    members = _dev(members, torch.int32)
    for name, t in (("q_song", q_song), ("members", members)):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
            raise ValueError("%s must lie in [0, %d)" % (name, n))
    out = torch.empty(members.numel(), dtype=torch.int32, device="cuda")
    rc = lib.acoss_eval_ranks(_ptr(D), n, int(D.stride(0)), _ptr(pos), _ptr(q_song), _ptr(m_off), _ptr(members),
                              int(q_song.numel()), _ptr(out), _stream())
    _check(rc, "acoss_eval_ranks")
    return out.cpu().numpy()


def profile_enable(on=True):
    load_library().acoss_profile_enable(1 if on else 0)


def profile_read():
    """{phase name: (total_ms, launches)} for the phases recorded since profile_enable(True)."""
    lib = load_library()
    n = 32
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_int64 * n)()
    k = lib.acoss_profile_read(ms, cnt, n)
    if k < 0:
        _check(k, "acoss_profile_read")
    return {lib.acoss_profile_phase_name(i).decode(): (ms[i], int(cnt[i])) for i in range(k) if cnt[i] > 0}
