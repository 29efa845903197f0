"""acoss_earlyfusion_snf across the bank classes its host sizing and its CSM kernels choose from,
over pair lists whose tracks recur, and under chunkings between "whole list" and "one pair".

ef_launch_csms picks its kernels from ld = the bank's longest track (rounded up to 4), and the LDS
fusion's size classes come from n_fuse = min(101, 2 ld), so each bank here is a bank of its own:

  tiny   12, 16, 20 blocks, ld 20      2 ld = 40 < 45: c1 = c2 = n_fuse, the 256-thread LDS launch only,
                                       no workspace launches
  short  14, 22, 23, 31, 47, ld 48     32 x 32 wave tiles, k_ef_csm_w4, k_ef_csm_pack<2>; n = 45 | 46 (the
                                       256 | 512-thread class edge), n = 94 in the 1024-thread class with
                                       16 * 94^2 = 141,376 bytes of LDS (the attribute is set)
  mid    30, 64, 65, 101, 128, ld 128  pack<2> with 64 x 64 cosine tiles; LDS and workspace pairs in one
                                       chunk (n = 60 .. 256); n = 128, 129, 192, 256 (register-row edges of
                                       k_efs_rows)
  long   40, 300, 512, ld 512          one tile per pair; n = 1024 (all 16 row registers), 812 twice,
                                       and n = 80, an LDS pair in a bank whose ld is 512; niters = 1

tiny, short and mid run all T^2 ordered pairs: runs of one query (which k_ef_csm_pack packs), every
track in 2 T pairs, both orders, self pairs (sa == sb), U < 2 P in every chunk. The features are
integer-exact (early_snf_cases.EXACT). The short and mid classes run a second bank each of general
float32 features (early_snf_cases.FLOAT), whose restatement starts from oracle.ef_csm's distances:
the kernels' CSM and self-distance bits must equal the canonical oracle's for those to pass.

Every run is compared with the numpy restatement by early_snf_cases.check_against_restatement: the
cross block within the pair's own measured bound (8 x the deviation between the restatement's two
evaluations; nothing measured on the GPU enters it), the score equal to Smith-Waterman of the run's
own cross, and equal to the restatement's on every stable pair.
"""
import numpy as np
import pytest

import early_snf_cases as ec

pytestmark = pytest.mark.gpu

K, KAPPA = ec.BANK_K, ec.BANK_KAPPA


def per_pair_bytes(ld, K):
    """The workspace bytes of one pair, restated from acoss_earlyfusion_snf (ef_snf.hip, `per_pair`),
    mat = ld^2, ldn = 2 ld, n2 = ldn^2, wplane = ceil(ld / 16) ld u16 words:
        3 mat 4 + 2 3 mat 4   the CSMs and the self distances of two tracks
        3 4 ld 4              the four k-smallest means per feature
        7 n2 8                six running planes and B
        3 K ldn 12            the neighbour lists (int32 J, float64 V)
        mat 8 + wplane 2      the cross plane and the bit plane
        sw_b + 64             the Smith-Waterman scratch: 32 bytes up to 512 rows (one band)
    about 268 ld^2 + 72 K ld."""
    assert ld <= 512
    mat, ldn = ld * ld, 2 * ld
    return (3 * mat * 4 + 2 * 3 * mat * 4 + 3 * 4 * ld * 4 + 7 * ldn * ldn * 8 + 3 * K * ldn * 12 + mat * 8 +
            (ld + 15) // 16 * ld * 2 + 32 + 64)


def chunk_of(budget, ld, K, n_pairs):
    return min(n_pairs, max(1, min(32768, budget // per_pair_bytes(ld, K))))


@pytest.fixture(scope="module", params=["tiny", "short", "mid", "long"])
def bank_run(request):
    """(name, case, bank, the run of the whole list)."""
    name = request.param
    feats, pairs, refs = ec.bank_case(name)
    bank, _ = ec.make_bank(feats)
    ld = (bank["max_blocks"] + 3) // 4 * 4
    assert ld == {"tiny": 20, "short": 48, "mid": 128, "long": 512}[name]
    niters = ec.BANKS[name][2]
    return name, (feats, pairs, refs), bank, niters, ec.run_snf(bank, pairs, KAPPA, K, niters)


def test_bank_against_restatement(bank_run):
    name, (feats, pairs, refs), _, _, whole = bank_run
    assert all(r["bound"] is not None for r in refs)  # K = 10 fuses every pair of these banks
    # the long bank's (300, 512) need not be stable under the restatement alone: no share asked there
    ec.check_against_restatement(feats, pairs, refs, whole, KAPPA, share=0.0 if name == "long" else 0.7, label=name)


def test_same_bits_in_any_order_and_chunking(bank_run, monkeypatch):
    """The whole list, a seeded permutation of it, and two budgets that cut it into chunks of 2 and of
    4 pairs (ragged last chunk; tracks recur within and across chunks): the same bits. The number of
    chunks each run really used is read from the phase profile: acoss_earlyfusion_snf opens its "snf"
    phase once per chunk."""
    from acoss import _lib
    name, (feats, pairs, refs), bank, niters, whole = bank_run
    P = len(pairs)
    ld = (bank["max_blocks"] + 3) // 4 * 4

    def counted(pp):
        _lib.profile_enable(True)
        try:
            got = ec.run_snf(bank, pp, KAPPA, K, niters)
            return got, _lib.profile_read()["snf"][1]
        finally:
            _lib.profile_enable(False)

    monkeypatch.delenv("ACOSS_EF_BYTES", raising=False)
    got, chunks = counted(pairs)
    assert chunks == 1 and ec.same_bits(got, whole)
    perm = np.random.default_rng(5).permutation(P)
    (sp, cp), chunks = counted(pairs[perm])
    inv = np.argsort(perm)
    assert chunks == 1 and ec.same_bits((sp[inv], [cp[i] for i in inv]), whole)
    seen = {1}
    for pairs_per_chunk in (2.5, 4.5):
        budget = int(pairs_per_chunk * per_pair_bytes(ld, K))
        chunk = chunk_of(budget, ld, K, P)
        assert chunk == min(P, int(pairs_per_chunk))
        monkeypatch.setenv("ACOSS_EF_BYTES", str(budget))
        got, chunks = counted(pairs)
        assert chunks == -(-P // chunk), (name, chunks, chunk)
        assert ec.same_bits(got, whole), (name, budget)
        seen.add(chunks)
    # the runs really differed in their chunking: 25 pairs in 1, 13 and 7 chunks (tiny: 9 in 1, 5, 3)
    assert seen == {1, -(-P // 2), -(-P // 4)} and len(seen) == (3 if P > 4 else 2)


def test_scores_without_cross(bank_run):
    name, (_, pairs, _), bank, niters, whole = bank_run
    score, cross = ec.run_snf(bank, pairs, KAPPA, K, niters, want_cross=False)
    assert cross is None and np.array_equal(score, whole[0], equal_nan=True)


@pytest.mark.parametrize("lds_n", [30, 50, 64])
def test_short_bank_lds_classes_same_bits(lds_n, monkeypatch):
    """ACOSS_EFS_LDS_N moves pairs between the LDS size classes and the workspace kernels: 30 leaves
    c1 = c2 = n_fuse = 30 (n = 28 only in LDS), 50 makes c2 = n_fuse = 50 (no third launch), 64 ends
    the LDS regime at the 512-thread class. The short bank's n run from 28 to 94."""
    feats, pairs, _ = ec.bank_case("short")
    bank, _ = ec.make_bank(feats)
    monkeypatch.delenv("ACOSS_EFS_LDS_N", raising=False)
    whole = ec.run_snf(bank, pairs, KAPPA, K, 5)
    monkeypatch.setenv("ACOSS_EFS_LDS_N", str(lds_n))
    assert ec.same_bits(ec.run_snf(bank, pairs, KAPPA, K, 5), whole)


@pytest.mark.parametrize("name", ["short", "mid"])
def test_float_bank_against_restatement(name):
    """General float32 features: the restatement runs on oracle.ef_csm's distances (canonical order)."""
    feats, pairs, refs = ec.float_case(name)
    bank, _ = ec.make_bank(feats)
    assert (bank["max_blocks"] + 3) // 4 * 4 == {"short": 48, "mid": 128}[name]
    got = ec.run_snf(bank, pairs, KAPPA, K, 5)
    ec.check_against_restatement(feats, pairs, refs, got, KAPPA, label="float-" + name)
