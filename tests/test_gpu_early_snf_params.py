"""acoss_earlyfusion_snf over its parameters: K, niters, mu, reg_diag, kappa, one GPU call per row
over seven pairs of one bank (ld = 72; n = 45 .. 134: all three LDS size classes and the workspace
kernels), each compared with the numpy restatement as test_gpu_early_snf_banks.py does.

  K = 2, 3, 11      k1 = k2 = 1; odd and uneven splits; NaN where the reference refuses the pair
  K = 50, 64        above the shorter tracks' block counts, and the lane limit of k_efs_rows
  niters = 1, 2     the first round only (reads P, writes the second planes); the first in-place round
  mu = 0.3, 1.0
  reg_diag = 0, .25 the `reg_diag > 0` branch off; a value other than 1
  kappa = .3, 3, 0  rint(kappa N); an integer count; every cell a one

K is held to [1, 64] whatever the bank's max_blocks is (each pair answers for K on its own): on a bank
of two 40-block tracks K = 50 and K = 64 return scores; 65 and a 513-block bank are ACOSS_E_ARG.
"""
import ctypes

import numpy as np
import pytest

import early_snf_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def param_bank():
    feats, _, _ = ec.param_tracks()
    bank, _ = ec.make_bank(feats)
    assert (bank["max_blocks"] + 3) // 4 * 4 == 72
    return bank


@pytest.mark.parametrize("row", ec.PARAM_ROWS, ids=ec.row_id)
def test_row_against_restatement(param_bank, row):
    feats, pairs, refs = ec.param_case(row)
    refused = [ec.PARAM_SHAPES[p] for p, r in enumerate(refs) if r["bound"] is None]
    assert refused == ec.PARAM_REFUSED.get(row.K, [])
    got = ec.run_snf(param_bank, pairs, row.kappa, row.K, row.niters, row.mu, row.reg_diag)
    ec.check_against_restatement(feats, pairs, refs, got, row.kappa, label=ec.row_id(row))


@pytest.mark.parametrize("K", [50, 64])
def test_k_above_max_blocks_fuses(K):
    feats, pairs, refs = ec.k_above_blocks_case(K)
    bank, _ = ec.make_bank(feats)
    assert bank["max_blocks"] == 40 < K and refs[0]["stable"]
    got = ec.run_snf(bank, pairs, ec.BANK_KAPPA, K, 5)
    ec.check_against_restatement(feats, pairs, refs, got, ec.BANK_KAPPA, label="K%d on 40 blocks" % K)


def test_raw_call_refuses_k_65_and_513_blocks():
    import torch
    from acoss import _lib
    feats, pairs, _ = ec.k_above_blocks_case(50)
    bank, _ = ec.make_bank(feats)
    lib = _lib.load_library()
    pd = torch.as_tensor(pairs).cuda()
    sc = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")

    def raw(K, max_blocks):
        return lib.acoss_earlyfusion_snf(_lib._ptr(bank["mfccs"]), _lib._ptr(bank["ssms"]), _lib._ptr(bank["chromas"]),
                                         _lib._ptr(bank["chroma_med"]), _lib._ptr(bank["off"]), _lib._ptr(bank["nb"]),
                                         len(feats), max_blocks, 1000, 1225, 480, _lib._ptr(pd), 1, ec.BANK_KAPPA, K, 0.5,
                                         5, 1.0, _lib._ptr(sc), None, 0, None,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert raw(65, 40) == -1 and b"acoss_earlyfusion_snf" in lib.acoss_last_error()
    assert raw(0, 40) == -1
    assert raw(10, 513) == -1 and b"512" in lib.acoss_last_error()
    assert float(sc[0]) == 7.0  # nothing written by the refused calls
    assert raw(64, 40) == 0 and np.isfinite(float(sc[0])) and float(sc[0]) != 7.0
    # the four scores keep their own rule: getWCSM(K, K) needs K <= max_blocks
    four = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    rc = lib.acoss_earlyfusion(_lib._ptr(bank["mfccs"]), _lib._ptr(bank["ssms"]), _lib._ptr(bank["chromas"]),
                               _lib._ptr(bank["chroma_med"]), _lib._ptr(bank["off"]), _lib._ptr(bank["nb"]), len(feats), 40,
                               1000, 1225, 480, _lib._ptr(pd), 1, ec.BANK_KAPPA, 41, 0.5, _lib._ptr(four),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and b"acoss_earlyfusion: bad arguments" in lib.acoss_last_error()
    assert bool((four == 7.0).all())


def test_duplicate_blocks_stay_finite():
    """A track of twelve identical blocks against an ordinary one, both ways: its self distances are
    all zero, so getW's MeanDist is 0 and Denom = 0 -> 1 (w_ssm's `den == 0`)."""
    feats, pairs, refs = ec.duplicate_block_case()
    bank, _ = ec.make_bank(feats)
    got = ec.run_snf(bank, pairs, ec.BANK_KAPPA, ec.BANK_K, 5)
    ec.check_against_restatement(feats, pairs, refs, got, ec.BANK_KAPPA, share=0.0, label="duplicate blocks")
