"""GPU parity of the Serra09/Chen CRP path off its default parameters, against the CPU oracle.

Single pairs (acoss_crp_pair): the threshold selects over a kappa sweep (kappa = 0, 1 and
integer (n-1) kappa included) on inputs whose lines hold exact tie groups of every size the
selects branch on; tests/test_crp_select_cases.py checks on the CPU that these inputs reach every
branch class at every line type, and that the oracle's percentile equals a numpy restatement.
Batches (acoss_crp_align): kappa, oti, the gap penalties and (m, tau) through the grouped, fast,
general and packed DP kernels. Every comparison is exact (==, thresholds by their bits).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import crp_cases
import oracle
from acoss import _lib, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# m = 9, tau = 1 (the split kernels): one shape per line type of the selects, and two where lines
# of at most 512 codes run inside a long-line and a Line2 launch.
@pytest.mark.parametrize("pairing", crp_cases.PAIRINGS)
@pytest.mark.parametrize("shape", list(crp_cases.LINE_SHAPES) + list(crp_cases.MIXED_SHAPES), ids=lambda s: "%dx%d" % s)
def test_crp_pair_kappa_sweep(shape, pairing):
    crp_cases.check_pair_on_gpu(shape[0], shape[1], pairing, crp_cases.kappas_for(*shape))


# The generic kernels (block_percentile of crp.hip) on the same kind of input: the run tracks still
# give large tie groups at these stackings (a run of g + 8 frames is g + 9 - m equal stacked
# frames at tau = 1; at tau = 2 the groups are shorter, ties remain).
@pytest.mark.parametrize("m,tau", [(4, 1), (9, 2)])
def test_crp_pair_kappa_sweep_generic(m, tau):
    crp_cases.check_pair_on_gpu(523, 611, "runs_x_runs", crp_cases.KAPPAS, m=m, tau=tau)


def test_crp_pair_kappa_sweep_no_short():
    """The 700 x 1000 cases with the lane-strided short-line selects switched off
    (ACOSS_NO_SHORT, read once per process: hence the subprocess)."""
    code = ("import sys; sys.path[:0] = %r\n"
            "import crp_cases\n"
            "for pairing in crp_cases.PAIRINGS:\n"
            "    crp_cases.check_pair_on_gpu(700, 1000, pairing, crp_cases.kappas_for(700, 1000))\n"
            "print('ok')\n" % [ROOT, os.path.join(ROOT, "acoss-1_amd"), os.path.join(ROOT, "tests")])
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ACOSS_NO_SHORT="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------
# Batches
# ------------------------------------------------------------------------------------------
def _corpus(lengths, seed, runs, silent):
    """synthetic.render tracks of the given lengths; those at the indices `runs` are run tracks
    (crp_cases.run_track), the one at `silent` carries a silence over [n/6, n/2)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    alphabet = crp_cases.make_alphabet(rng)
    tracks = []
    for t, n in enumerate(lengths):
        if t in runs:
            x = crp_cases.run_track(rng, n, crp_cases.SIZES, alphabet)
        else:
            x = crp_cases.natural_track(rng, n)
        if t == silent:
            x[n // 6:n // 2] = 0.0
        tracks.append(x)
    return tracks


def _all_pairs(idx):
    return np.array([(i, j) for i in idx for j in idx if i != j], np.int32)


def _check_batch(tracks, idx, ref, ref_pairs, **params):
    """crp_align over all ordered pairs of tracks[idx] (packed on their own, so the launch's
    longest line is theirs) == the oracle's results of the same pairs."""
    sub = [tracks[i] for i in idx]
    feats, off, lens = synthetic.pack(sub)
    pairs = _all_pairs(range(len(idx)))
    got = _lib.crp_align(feats, off, lens, int(lens.max()), pairs, _lib.crp_params(**params), qmax=True, dmax=True,
                         oti=True)
    pos = {(int(a), int(b)): n for n, (a, b) in enumerate(ref_pairs)}
    sel = np.array([pos[(idx[a], idx[b])] for a, b in pairs])
    q, d, k = ref
    np.testing.assert_array_equal(got["oti"].cpu().numpy(), k[sel])
    np.testing.assert_array_equal(got["qmax"].cpu().numpy(), q[sel])
    np.testing.assert_array_equal(got["dmax"].cpu().numpy(), d[sel])


# A: every line at most 512 codes: LineS<8> selects, the grouped Qmax DP with 4 pairs per wave.
# B: lines up to 2048 codes: as one launch the 32-rows-per-lane DP and the packed chen17 DP; its
#    four shortest tracks alone (lines of 521..672 codes) the grouped DP with 3 pairs per wave and
#    the 16-rows-per-lane dmax DP.
CORPORA = {"A": dict(lengths=[10, 41, 120, 250, 400, 505], seed=21, runs=(2, 4), silent=3, subsets=()),
           "B": dict(lengths=[300, 530, 610, 681, 1500, 2057], seed=22, runs=(1, 4), silent=2, subsets=((0, 1, 2, 3),))}

# kappa = 0 / 1: the minimum / the maximum (kappa = 1: all-ones masks, the largest score growth the
# packed 16-bit DP must hold). gamma_open == gamma_ext = K/2 with K = 0, 2, 3 in the grouped, fast
# and packed kernels; 0.25: equal penalties whose double is no integer, and unequal penalties (the
# general DP, EQG true / false).
PARAM_SETS = [dict(kappa=0.0), dict(kappa=1.0), dict(kappa=0.3), dict(oti=False),
              dict(gamma_open=0.0, gamma_ext=0.0), dict(gamma_open=1.0, gamma_ext=1.0),
              dict(gamma_open=1.5, gamma_ext=1.5), dict(gamma_open=0.25, gamma_ext=0.25),
              dict(gamma_open=0.7, gamma_ext=0.3)]


@pytest.mark.parametrize("params", PARAM_SETS, ids=lambda p: ",".join("%s=%g" % kv for kv in p.items()))
@pytest.mark.parametrize("name", list(CORPORA))
def test_crp_align_params(name, params):
    c = CORPORA[name]
    tracks = _corpus(c["lengths"], c["seed"], c["runs"], c["silent"])
    feats, off, lens = synthetic.pack(tracks)
    everyone = tuple(range(len(tracks)))
    ref_pairs = _all_pairs(everyone)
    ref = oracle.crp_batch(feats, off, lens, ref_pairs, **params)
    for idx in (everyone,) + c["subsets"]:
        _check_batch(tracks, idx, ref, ref_pairs, **params)


# (m, tau) off (9, 1): the generic kernels as a batch. The first track is one frame longer than
# the stacking needs: CRPs of one row / one column.
@pytest.mark.parametrize("m,tau,lengths", [(1, 1, [2, 64, 200, 333, 700]), (4, 2, [9, 64, 200, 333, 700]),
                                           (9, 3, [28, 64, 200, 333, 700]), (64, 1, [65, 130, 200, 333, 700])])
def test_crp_align_generic_batch(m, tau, lengths):
    assert lengths[0] == m * tau + 1 and oracle.stacked_len(lengths[0], m, tau) == 1
    tracks = _corpus(lengths, 23 + m, runs=(2,), silent=3)
    feats, off, lens = synthetic.pack(tracks)
    everyone = tuple(range(len(tracks)))
    ref_pairs = _all_pairs(everyone)
    ref = oracle.crp_batch(feats, off, lens, ref_pairs, m=m, tau=tau)
    _check_batch(tracks, everyone, ref, ref_pairs, m=m, tau=tau)


# ------------------------------------------------------------------------------------------
# Refusals
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,names", [(dict(kappa=-0.01), "kappa=-0.01"), (dict(kappa=1.01), "kappa=1.01"),
                                       (dict(kappa=float("nan")), "kappa=nan"), (dict(m=0), "m=0 "),
                                       (dict(m=65), "m=65 "), (dict(tau=0), "tau=0 ")])
def test_crp_params_refused(bad, names):
    """check_params refuses before anything is launched: both entry points raise, and
    acoss_last_error names the parameters."""
    rng = np.random.Generator(np.random.PCG64(3))
    tracks = [crp_cases.natural_track(rng, n) for n in (120, 150)]
    feats, off, lens = synthetic.pack(tracks)
    params = _lib.crp_params(**bad)
    full = "unsupported params m=%d tau=%d kappa=%g" % (params.m, params.tau, params.kappa)
    assert names in full + " "
    with pytest.raises(_lib.AcossHipError, match="ACOSS_E_ARG") as e:
        _lib.crp_align(feats, off, lens, int(lens.max()), np.array([(0, 1)], np.int32), params, qmax=True, dmax=True,
                       oti=True)
    assert _lib.load_library().acoss_last_error().decode() == full
    assert full in str(e.value)
    if params.tau > 0:  # (the Python wrapper sizes the outputs by tau before it calls in)
        with pytest.raises(_lib.AcossHipError, match="ACOSS_E_ARG") as e:
            _lib.crp_pair(tracks[0], tracks[1], params)
        assert full in str(e.value)
    # the library is usable afterwards and the error text is cleared by the next good call
    got = _lib.crp_align(feats, off, lens, int(lens.max()), np.array([(0, 1)], np.int32), _lib.crp_params())
    assert _lib.load_library().acoss_last_error().decode() == ""
    assert got["qmax"].cpu().numpy() == oracle.crp_batch(feats, off, lens, np.array([(0, 1)], np.int32))[0]
