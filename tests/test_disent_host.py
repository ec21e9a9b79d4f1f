"""CPU-only checks of the device-side disentanglement scores: the new entry points are declared, bound and exported
alike (and refuse what lies outside their range before any launch), ``FactorSampler`` indexes and draws as documented,
and a numpy fp64 restatement of the scores' rule -- written here, shared with tests/test_hip_disent.py -- reproduces the
results recorded from the unmodified reference (tests/golden/disent.npz).  The histogram's launch plan is restated too
(``ref_hist_tiling``) and held to the library's own planner (``itcv_disent_hist_tiling``, no GPU work) on the table of
tiers the GPU tests launch (``HIST_TIERS``), on the earlier tests' shapes and over a random sweep."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("itcv_disent_minmax_workspace", "itcv_disent_minmax", "itcv_disent_bins", "itcv_disent_counts_elems",
       "itcv_disent_hist", "itcv_disent_mi")


# ---- the rule, restated in numpy fp64 (include/itcv_hip.h; evaluation/utils.py:245-273,323-335 of the reference) ----
def ref_bins(x, bins):
    """bin(x) = #{j in 0..bins-1 : x >= lo + j * ((hi - lo) / bins)} per column, lo -= 0.5 / hi += 0.5 when equal."""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros(x.shape, dtype=np.int32)
    for d in range(x.shape[1]):
        col = x[:, d].astype(np.float64)
        lo, hi = col.min(), col.max()
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        w = (hi - lo) / bins
        for j in range(bins):
            out[:, d] += col >= lo + j * w
    return out


def ref_counts(b, v, sizes, bins):
    """(list of K arrays [D, bins, size_k], list of K marginals [size_k]) from bins in 1..bins and factor values."""
    N, D = b.shape
    joint, marg = [], []
    for k, s in enumerate(sizes):
        t = np.zeros((D, bins, s), dtype=np.int64)
        for d in range(D):
            np.add.at(t[d], (b[:, d] - 1, v[:, k]), 1)
        joint.append(t)
        marg.append(np.bincount(v[:, k], minlength=s).astype(np.int64))
    return joint, marg


def ref_mi(joint, marg, N):
    """MI[d, k] = max(0, sum_{c>0} (c/N)(log c - log r_b - log s_f + log N)), H[k] = sum_{s>0} -(s/N) log(s/N)."""
    D, K = joint[0].shape[0], len(joint)
    mi, h = np.zeros((D, K)), np.zeros(K)
    for k in range(K):
        for d in range(D):
            c = joint[k][d].astype(np.float64)
            r, s = c.sum(1, keepdims=True), c.sum(0, keepdims=True)
            nz = c > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (c / N) * (np.log(c) - np.log(r) - np.log(s) + np.log(float(N)))
            mi[d, k] = max(0.0, float(t[nz].sum()))
        p = marg[k][marg[k] > 0] / N
        h[k] = float((-p * np.log(p)).sum())
    return mi, h


def ref_mig(mi, h):
    top = np.sort(mi, axis=0)[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.mean((top[0] - top[1]) / h))


def ref_modularity(mi):
    theta = mi.max(1)
    t = np.zeros_like(mi)
    t[np.arange(mi.shape[0]), mi.argmax(1)] = theta
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.mean(1 - ((mi - t) ** 2).sum(1) / (theta ** 2 * (mi.shape[1] - 1))))


def ref_all(x, v, sizes, bins):
    b = ref_bins(x, bins)
    joint, marg = ref_counts(b, np.asarray(v), sizes, bins)
    mi, h = ref_mi(joint, marg, len(b))
    return b, joint, marg, mi, h


# ---- the histogram's launch plan (hist_plan of csrc/disent.hip), restated --------------------------------------------
def ref_hist_tiling(D, sizes, bins):
    """A block's table, (tc * bins + 1) * gsum words, must fit 64 KiB: consecutive factors are grouped greedily against the
    words one column needs, then the column tile is halved from 64 while it is wider than needed or does not fit."""
    cap = 16384 // (bins + 1)
    groups, gs, gmax = [0], 0, 0
    for k, s in enumerate(sizes):
        if gs and gs + s > cap:
            groups.append(k)
            gs = 0
        gs += s
        gmax = max(gmax, gs)
    t = 64
    while t > 1 and (t // 2 >= D or (t * bins + 1) * gmax * 4 > 65536):
        t //= 2
    return dict(tc=t, column_tiles=-(-D // t), groups=groups, lds_bytes=(t * bins + 1) * gmax * 4)


# name: (D, factor sizes, bins, columns per block, column tiles, width of the last tile, factor groups, LDS bytes).
# The tiers tests/test_hip_disent.py launches at N = 1037; "large_n" is its N = 262 445 case.
HIST_TIERS = {
    "tc64": (70, (6, 6, 2, 3, 3), 10, 64, 2, 6, [0], 51280),
    "tc32": (70, (6, 6, 2, 3, 3), 20, 32, 3, 6, [0], 51280),
    "tc4_dsprites": (10, (3, 6, 40, 32, 32), 20, 4, 3, 2, [0], 36612),
    "tc2": (5, (100, 100), 32, 2, 3, 1, [0], 52000),
    "tc2_groups": (5, (250, 250, 250), 32, 2, 3, 1, [0, 1, 2], 65000),
    "tc1_wide": (3, (200, 200), 32, 1, 3, 1, [0], 52800),
    "large_n": (5, (3, 7), 20, 8, 1, 5, [0], 6440),
}
# the shapes of the tests that came with the kernels: (D, factor sizes, bins, columns per block, factor groups)
HIST_EARLIER = [
    (10, (6, 6, 2, 3, 3, 40, 40), 10, 16, 1), (10, (6, 6, 2, 3, 3, 40, 40), 20, 8, 1), (9, (6, 6, 2, 3, 3, 40, 40), 20, 8, 1),
    (1, (3,), 10, 1, 1), (1, (2,), 1, 1, 1), (1, (2,), 2, 1, 1), (1, (2,), 32, 1, 1), (2, (2, 1), 10, 2, 1),
    (129, (2, 3, 256, 5, 1, 7, 4, 9, 2, 6, 3, 8, 2, 5, 4, 3), 32, 1, 1), (3, (256,) * 16, 32, 1, 16), (10, (4, 5), 10, 16, 1),
    (10, (4, 5), 20, 16, 1)]


@pytest.mark.parametrize("name", sorted(HIST_TIERS))
def test_hist_tiling_query_restatement_and_case_table_agree(name):
    from hipvae import functional as HF
    D, sizes, bins, tc, tiles, last, groups, lds = HIST_TIERS[name]
    want = dict(tc=tc, column_tiles=tiles, groups=groups, lds_bytes=lds)
    assert ref_hist_tiling(D, sizes, bins) == want
    assert HF.disent_hist_tiling(D, sizes, bins) == want
    assert D - (tiles - 1) * tc == last and lds <= 65536


def test_hist_tiling_on_the_earlier_shapes_and_over_a_sweep():
    from hipvae import functional as HF
    for D, sizes, bins, tc, ng in HIST_EARLIER:
        got = HF.disent_hist_tiling(D, sizes, bins)
        assert got == ref_hist_tiling(D, sizes, bins), (D, sizes, bins)
        assert (got["tc"], len(got["groups"])) == (tc, ng), (D, sizes, bins, got)
    # what the earlier shapes never launched (2 is reached by the N = 1 edge case alone, with one row)
    assert sorted({t[3] for t in HIST_EARLIER}) == [1, 2, 8, 16]
    assert sorted({t[3] for t in HIST_TIERS.values()}) == [1, 2, 4, 8, 32, 64]
    rs = np.random.RandomState(0)
    for _ in range(300):
        D, bins, K = int(rs.randint(1, 200)), int(rs.randint(1, 33)), int(rs.randint(1, 17))
        sizes = [int(s) for s in rs.randint(1, 257, size=K)]
        got = HF.disent_hist_tiling(D, sizes, bins)
        assert got == ref_hist_tiling(D, sizes, bins), (D, sizes, bins)
        # more than one group leaves room for two columns at the most: a group is closed only when the next factor would
        # pass 16384 // (bins + 1) words, so the largest group holds more than half of that
        assert got["lds_bytes"] <= 65536 and (len(got["groups"]) == 1 or got["tc"] <= 2)


def test_hist_tiling_query_refuses_what_the_histogram_refuses():
    from hipvae import abi
    from hipvae import functional as HF
    out = (ctypes.c_int * 21)()
    for K, sizes, bins, msg in [(2, (4, 5), 33, "bins = 33"), (2, (4, 257), 10, "size 257"), (17, (2,) * 17, 10, "K = 17")]:
        assert abi.lib.itcv_disent_hist_tiling(8, K, _sizes(*sizes), bins, out) != 0
        assert abi.last_error().startswith("itcv_disent_hist_tiling") and msg in abi.last_error(), abi.last_error()
    assert abi.lib.itcv_disent_hist_tiling(0, 2, _sizes(4, 5), 10, out) != 0
    assert abi.lib.itcv_disent_hist_tiling(8, 2, None, 10, out) != 0 and abi.lib.itcv_disent_hist_tiling(8, 2, _sizes(4, 5), 10, None) != 0
    with pytest.raises(RuntimeError, match="bins = 0"):
        HF.disent_hist_tiling(8, (4, 5), 0)
    assert "itcv_disent_hist_tiling" in abi.SIGNATURES and abi.ABI_VERSION == 4


# ---- boundary ------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_and_library():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert abi.ABI_VERSION == 4 == lib.itcv_abi_version()
    assert re.search(r"#define ITCV_ABI_VERSION 4\b", header)


A, B, C, D_, E, F, G = (0x10000 * i for i in range(1, 8))     # fake device addresses: every call fails before a launch


def _sizes(*s):
    return (ctypes.c_int * len(s))(*s)


@pytest.mark.parametrize("K, sizes, bins, msg", [
    (2, (4, 5), 33, "bins = 33"), (2, (4, 5), 0, "bins = 0"), (2, (4, 257), 10, "size 257"), (2, (0, 5), 10, "size 0"),
    (17, (2,) * 17, 10, "K = 17"), (0, (), 10, "K = 0")])
def test_range_checks_fail_before_any_launch(K, sizes, bins, msg):
    from hipvae import abi
    rc = abi.lib.itcv_disent_hist(A, 8, B, 100, 8, K, _sizes(*sizes) if sizes else _sizes(1), bins, C, D_, E, F, G, None)
    assert rc != 0 and abi.last_error().startswith("itcv_disent_hist") and msg in abi.last_error(), abi.last_error()
    rc = abi.lib.itcv_disent_mi(E, F, 100, 8, K, _sizes(*sizes) if sizes else _sizes(1), bins, C, D_, None)
    assert rc != 0 and msg in abi.last_error(), abi.last_error()
    with pytest.raises(RuntimeError):
        abi.call("itcv_disent_mi", E, F, 100, 8, K, _sizes(*sizes) if sizes else _sizes(1), bins, C, D_, None)


def test_argument_checks_and_size_queries():
    from hipvae import abi
    assert abi.lib.itcv_disent_bins(A, 8, 10, 8, B, C, 33, D_, None) != 0 and "bins = 33" in abi.last_error()
    assert abi.lib.itcv_disent_bins(A, 4, 10, 8, B, C, 10, D_, None) != 0           # row stride below D
    assert abi.lib.itcv_disent_minmax(A, 8, 0, 8, B, C, D_, E, 1 << 20, None) != 0  # N = 0
    assert abi.lib.itcv_disent_minmax(A, 8, 10, 8, B, C, D_, None, 0, None) != 0    # no workspace
    assert "workspace" in abi.last_error()
    assert abi.lib.itcv_disent_counts_elems(10, 100, 20) == 10 * 100 * 20
    assert abi.lib.itcv_disent_counts_elems(0, 100, 20) == 0
    assert abi.lib.itcv_disent_minmax_workspace(256, 10) == 2 * 1 * 10 * 4
    assert abi.lib.itcv_disent_minmax_workspace(10000, 128) == 2 * 40 * 128 * 4
    assert abi.lib.itcv_disent_minmax_workspace(1 << 30, 3) == 2 * 1024 * 3 * 4     # slices are capped, rows grow
    from hipvae import disentangle, functional
    with pytest.raises(abi.HipExtensionError):                                      # no CPU path
        disentangle.mig_score(torch.zeros(4, 3), torch.zeros(4, 2, dtype=torch.int32), [2, 2])
    with pytest.raises(abi.HipExtensionError):
        functional.disent_minmax(torch.zeros(4, 3, dtype=torch.float64), None)


# ---- FactorSampler -------------------------------------------------------------------------------------------------
class IndexDataset:
    """Item i is (a 1-element tensor holding i, None): what the sampler looked up is visible in its output."""
    factor_sizes = [3, 4, 1, 5]
    latent_indices = [0, 3]          # factor 1 (size 4) is observed, factor 2 has one value

    def __len__(self):
        return 60

    def __getitem__(self, i):
        assert 0 <= i < 60
        return torch.tensor([float(i)]), None


def test_factor_sampler_mixed_radix_lookup():
    from hipvae.disentangle import FactorSampler
    s = FactorSampler(IndexDataset(), torch.device("cpu"), seed=5)
    assert (s.factor_sizes, s.latent_indices, s.num_latents) == ([3, 4, 1, 5], [0, 3], 2)
    f = s.sample_factors_of_variation(200)
    assert f.shape == (200, 2) and set(f[:, 0]) == {0, 1, 2} and set(f[:, 1]) == {0, 1, 2, 3, 4}
    obs = s.sample_observations_from_factors(f)
    assert obs.shape == (200, 1)
    idx = obs[:, 0].numpy().astype(np.int64)
    # most significant factor first: idx = ((f0 * 4 + f1) * 1 + f2) * 5 + f3
    f3, rest = idx % 5, idx // 5
    f2, rest = rest % 1, rest // 1
    f1, f0 = rest % 4, rest // 4
    assert np.array_equal(f0, f[:, 0]) and np.array_equal(f3, f[:, 1]) and not f2.any()
    assert set(f1) == {0, 1, 2, 3}                       # the observed factor is filled at random over its range
    assert np.array_equal(s.indices_from_factors(np.array([[2, 4]])) // 20, [2])
    full = np.array([[2, 4]])
    assert int(s.indices_from_factors(full)[0]) % 5 == 4


def test_factor_sampler_seed_and_batches():
    from hipvae.disentangle import FactorSampler
    a = FactorSampler(IndexDataset(), torch.device("cpu"), seed=11)
    b = FactorSampler(IndexDataset(), torch.device("cpu"), seed=11)
    c = FactorSampler(IndexDataset(), torch.device("cpu"), seed=12)
    state = torch.get_rng_state()
    ga, gb, gc = (list(s.generate(20, 8)) for s in (a, b, c))
    assert torch.equal(torch.get_rng_state(), state)     # a private numpy generator: torch's is not consumed
    assert [len(f) for f, _ in ga] == [8, 8, 4] and [o.shape[0] for _, o in ga] == [8, 8, 4]
    for (fa, oa), (fb, ob) in zip(ga, gb):
        assert np.array_equal(fa, fb) and torch.equal(oa, ob)
    assert any(not np.array_equal(fa, fc) for (fa, _), (fc, _) in zip(ga, gc))
    assert [len(f) for f, _ in a.generate(20, 8, drop_last=True)] == [8, 8]
    assert [len(f) for f, _ in a.generate(16, 8)] == [8, 8]
    f, o = a.sample(3)
    assert f.shape == (3, 2) and o.shape == (3, 1)


# ---- the restatement against the reference's recorded results --------------------------------------------------------
def test_restatement_reproduces_the_reference():
    g = np.load(os.path.join(GOLDEN, "disent.npz"))
    x, v, sizes = g["x"], g["v"], [int(s) for s in g["sizes"]]
    assert x.shape == (777, 10) and x.dtype == np.float32 and sizes == [6, 6, 2, 3, 3, 40, 40]
    assert (x[:, -1] == np.float32(1.25)).all()
    res = {}
    for bins in (10, 20):
        b, joint, marg, mi, h = ref_all(x, v, sizes, bins)
        assert np.array_equal(b, g[f"bins{bins}"])                     # exactly
        assert np.abs(mi - g[f"MI{bins}"]).max() <= 1e-12
        assert np.abs(h - g["H"]).max() <= 1e-12
        assert all(t.sum() == 777 * 10 for t in joint)
        res[bins] = (mi, h)
    assert abs(ref_mig(*res[10]) - float(g["mig"])) <= 1e-12
    # the constant column knows nothing about any factor (theta = 0): 0 / 0, nan in the reference and here
    assert np.isnan(float(g["modularity"])) and np.isnan(ref_modularity(res[20][0]))
    assert abs(ref_modularity(res[20][0][:-1]) - float(g["modularity_informative"])) <= 1e-12
