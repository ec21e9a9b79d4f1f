"""CPU-only: the case tables of conv_cases.py do what they claim.  Every case's kernel instance is computed from the
library's host-only queries (``*_variant``, ``*_workspace``, ``*_supported``) and a few mirrored rules, the set of
instances each table reaches must be the full product of the template parameters, and every edge the tables are there
for is asserted by a predicate over them: deleting a case that alone provides an instance or an edge fails here, not
silently on the device."""
import itertools

import pytest

import conv_cases as cc


def _lib():
    from hipvae import abi
    return abi.lib


def _fwd(c):
    return cc.fwd_launch(_lib(), c.B, c.Ci, c.H, c.W, c.Co, c.KS, c.up2)


def _dgrad(c):
    return cc.fwd_launch(_lib(), c.B, c.Co, c.H, c.W, c.Ci, c.KS, 0)


def _wgrad(c):
    return cc.wgrad_launch(_lib(), c.B, c.Ci, c.H, c.W, c.Co, c.KS, c.up2)


def _has(table, pred):
    return any(pred(c) for _, c in cc.cases(table))


def test_mirrors_against_literals():
    lib = _lib()
    # (KS, BM, up2, tail, BN, mt, nt, ktiles, splits, kps)
    assert cc.fwd_launch(lib, 2, 16, 6, 10, 5, 1, 0) == (1, 32, 0, 0, 256, 1, 1, 1, 1, 1)
    assert cc.fwd_launch(lib, 3, 24, 20, 20, 130, 3, 0) == (3, 128, 0, 1, 128, 2, 10, 18, 4, 5)
    assert cc.fwd_launch(lib, 2, 24, 6, 10, 64, 3, 1) == (3, 64, 1, 1, 256, 1, 1, 18, 4, 5)
    assert cc.fwd_launch(lib, 2, 64, 4, 4, 8, 3, 0) == (3, 32, 0, 0, 256, 1, 1, 36, 9, 4)
    assert cc.fwd_launch(lib, 1, 528, 4, 4, 8, 5, 0) == (5, 32, 0, 0, 256, 1, 1, 825, 64, 13)
    assert cc.fwd_launch(lib, 2, 16, 64, 64, 260, 3, 0) == (3, 128, 0, 0, 128, 3, 64, 9, 1, 9)
    assert cc.fwd_launch(lib, 4, 512, 16, 16, 64, 3, 0)[7:] == (288, 58, 5)         # the cap of 64 before the slices are evened out
    # (KS, up2, CB, BM, swapped, ktiles, splits, kps, small reduce, W power of two, H*W power of two)
    assert cc.wgrad_launch(lib, 2, 64, 8, 8, 3, 5, 0) == (5, 0, 4, 64, 1, 4, 1, 4, 0, 1, 1)
    assert cc.wgrad_launch(lib, 2, 64, 8, 8, 3, 3, 1) == (3, 1, 64, 32, 0, 4, 1, 4, 0, 1, 1)
    assert cc.wgrad_launch(lib, 1, 200, 6, 10, 4, 3, 0) == (3, 0, 4, 128, 1, 2, 1, 2, 0, 0, 0)
    assert cc.wgrad_launch(lib, 6, 8, 20, 20, 16, 3, 0) == (3, 0, 16, 32, 0, 75, 9, 9, 0, 0, 0)
    assert cc.wgrad_launch(lib, 2, 3, 64, 74, 64, 5, 0) == (5, 0, 4, 64, 0, 296, 37, 8, 1, 0, 0)
    assert cc.wgrad_launch(lib, 2, 64, 64, 64, 3, 5, 0) == (5, 0, 4, 64, 1, 256, 32, 8, 1, 1, 1)
    assert cc.wgrad_launch(lib, 1, 3, 64, 74, 64, 5, 0)[6:9] == (17, 9, 0)          # fewer than 32 slices: the plain reduce
    assert cc.wgrad_launch(lib, 1, 24, 3, 8, 40, 3, 0)[9:] == (1, 0)
    assert [cc.col_block(n) for n in (1, 4, 5, 16, 17, 32, 33, 64, 65, 256)] == [4, 4, 16, 16, 32, 32, 64, 64, 128, 128]
    assert [cc.swapped(ci, co, u) for ci, co, u in ((5, 4, 0), (4, 4, 0), (5, 5, 0), (64, 3, 1))] == [True, False, False, False]
    assert [cc.tile_rows(n) for n in (1, 32, 33, 64, 65, 260)] == [32, 32, 64, 64, 128, 128]
    # the in-kernel-split kernels have no variant query: their mirrors restate plan_fwd(kFwdSplit) (no 32-row tile) and
    # plan_wgrad(min_bm = 64) and are pinned here as literals
    assert cc.split_fwd_instance(2, 32, 4, 8, 40, 1, 1, 2) == (1, 2, 64, 1)
    assert cc.split_fwd_instance(2, 64, 8, 8, 64, 3, 0, 3) == (3, 3, 64, 0)
    assert cc.split_fwd_instance(2, 64, 8, 8, 65, 3, 0, 3) == (3, 3, 128, 0)
    assert cc.split_wgrad_instance(2, 32, 8, 8, 33, 3, 2) == (3, 2, 32, 64)
    assert cc.split_wgrad_instance(2, 64, 8, 8, 64, 1, 3) == (1, 3, 64, 64)
    assert cc.split_wgrad_instance(2, 96, 8, 8, 65, 1, 3) == (1, 3, 128, 128)


def test_ids_name_the_launch():
    for table in cc.TABLES:
        assert len(set(cc.ids(table))) == len(cc.ids(table)), table
        assert len({c for _, c in cc.cases(table)}) == len(cc.ids(table)), table
    for cid, c in cc.cases("A"):
        f = _fwd(c)
        assert (cid + "-").startswith(f"k{f.KS}-m{f.BM}" + ("-up2" if f.up2 else "") + ("-tail-" if f.tail else "-")), cid
    for cid, c in cc.cases("B"):
        g = _wgrad(c)
        assert cid.startswith(f"k{g.KS}" + ("-up2" if g.up2 else "") + f"-c{g.CB}-m{g.BM}-"), cid
        assert ("swapped" in cid and "not-swapped" not in cid) == bool(g.swapped), cid
        assert ("small-reduce" in cid) == bool(g.small_reduce) and cid.endswith("-acc") == bool(c.accumulate), cid
    for cid, c in cc.cases("C_cout"):
        assert cid.startswith(f"out{c.KS}-{c.Co}-c{c.Ci}-{c.H}x{c.W}") and cid.endswith("-bias") == bool(c.bias), cid
    for cid, c in cc.cases("C_cin"):
        assert cid.startswith(f"in{c.KS}-{c.Ci}-co{c.Co}-{c.H}x{c.W}") and cid.endswith("-bias") == bool(c.bias), cid
    for cid, c in cc.cases("D"):
        bm = 64 if c.Co <= 64 else 128
        assert (cid + "-").startswith(f"k{c.KS}-m{bm}" + ("-up2-" if c.up2 else "-")), cid
        assert cid.endswith("-acc") == bool(c.accumulate), cid


def test_cases_are_accepted_by_their_entry_points():
    lib = _lib()
    pad16 = lambda n: cc.cdiv(n, 16) * 16
    for table in cc.TABLES:
        for cid, c in cc.cases(table):
            assert c.KS in (1, 3, 5) and min(c[:5]) >= 1 and (not c.up2 or (c.H % 2 == 0 and c.W % 2 == 0)), cid
            # check_dims: 31-bit buffer offsets, in both directions of the GEMM
            assert c.B * pad16(c.Ci) * c.H * c.W < 2 ** 29 and c.B * pad16(c.Co) * c.H * c.W < 2 ** 29, cid
    for cid, c in cc.cases("A"):
        f = _fwd(c)
        need = f.splits * c.B * c.Co * c.H * c.W * 4 if f.splits > 1 else 0
        assert lib.itcv_conv2d_fwd_workspace(c.B, c.Ci, c.H, c.W, c.Co, c.KS) == need, cid
    for cid, c in cc.cases("B"):
        g = _wgrad(c)
        ci, co = (c.Co, c.Ci) if g.swapped else (c.Ci, c.Co)
        kk = c.KS * c.KS
        nt = kk * cc.cdiv(ci, 128) if g.CB == 128 else cc.cdiv(kk, 128 // g.CB)
        need = g.splits * co * nt * 128 * 4                     # `splits` slabs of [rows][nt * 128]: pins the CB mirror
        have = lib.itcv_conv2d_wgrad_workspace(c.B, c.Ci, c.H, c.W, c.Co, c.KS)
        assert have >= need if (g.swapped or (c.Co <= 4 < c.Ci)) else have == need, cid
    for cid, c in cc.cases("C_cout"):
        assert lib.itcv_conv2d_small_cout_supported(c.Co, c.KS) and lib.itcv_conv2d_small_cin_supported(c.Co, c.KS), cid
        assert not c.up2 and not c.accumulate, cid
    for cid, c in cc.cases("C_cin"):
        assert lib.itcv_conv2d_small_cin_supported(c.Ci, c.KS) and lib.itcv_conv2d_small_cout_supported(c.Ci, c.KS), cid
        assert not c.up2 and not c.accumulate, cid
    for cid, c in cc.cases("D"):
        assert lib.itcv_conv2d_bf16s_supported(c.Ci, c.Co, c.KS), cid
        # (a width that is no multiple of 8 leaves the weight gradient on the fp32 kernel: one forward-only case)
        assert lib.itcv_conv2d_wgrad_bf16s_supported(c.Ci, c.H, c.W, c.Co, c.KS) == (c.W % 8 == 0), cid
    assert [cid for cid, c in cc.cases("D") if c.W % 8] == ["k1-m128-h1w1"]


def test_table_a_reaches_every_instance():
    reached = {(l.KS, l.BM, l.up2, l.tail) for _, c in cc.cases("A") for l in (_fwd(c), _dgrad(c))}
    assert reached == set(itertools.product((1, 3, 5), (32, 64, 128), (0, 1), (0, 1)))
    # the forward launches alone reach them all too: the ids name exactly those
    assert {(l.KS, l.BM, l.up2, l.tail) for l in (_fwd(c) for _, c in cc.cases("A"))} == reached


def test_table_a_edges():
    A = "A"
    # the K split and the path without it (bias added inside the kernel), each with and without bias
    assert {(_fwd(c).splits > 1, c.bias) for _, c in cc.cases(A)} == set(itertools.product((False, True), (0, 1)))
    for ks in (1, 3, 5):
        assert _has(A, lambda c: c.KS == ks and _fwd(c).splits == 1), ks
        assert _has(A, lambda c: c.KS == ks and _fwd(c).splits > 1), ks
    assert _has(A, lambda c: c.KS == 1 and c.Ci < 128 and _fwd(c).ktiles < 8 and _fwd(c).splits == 1)
    assert _has(A, lambda c: c.KS == 3 and _fwd(c).mt * _fwd(c).nt >= 192 and _fwd(c).splits == 1)
    assert _has(A, lambda c: c.KS == 5 and _fwd(c).mt * _fwd(c).nt >= 192 and _fwd(c).splits == 1)
    assert _has(A, lambda c: _fwd(c).splits > 1 and _fwd(c).ktiles % _fwd(c).kps)           # a short last slice
    assert _has(A, lambda c: _fwd(c).splits > 1 and _fwd(c).ktiles % _fwd(c).kps == 0)      # exactly even slices
    assert _has(A, lambda c: _fwd(c).splits == 64)                                          # the cap
    # pixel tails
    for bn in (128, 256):
        assert _has(A, lambda c: _fwd(c).BN == bn and (c.B * c.H * c.W) % bn), bn
        assert _has(A, lambda c: _fwd(c).BN == bn and c.B > 1 and (c.H * c.W) % bn and c.H * c.W < bn), bn   # a tile spans images
        assert _has(A, lambda c: _fwd(c).BN == bn and c.H * c.W > bn), bn
        # the padded grid of eight: blocks that return early, and a second group of eight
        assert _has(A, lambda c: _fwd(c).BN == bn and _fwd(c).nt % 8 and _fwd(c).nt > 8), bn
    assert _has(A, lambda c: (c.H, c.W) in ((6, 10), (5, 3)) and c.B > 1)
    # row tails and channel tails
    assert {1, 5, 33, 65, 129, 130} <= {c.Co for _, c in cc.cases(A)}
    assert {1, 17, 24, 16, 32} <= {c.Ci for _, c in cc.cases(A)}
    assert _has(A, lambda c: c.Ci == 24) and _has(A, lambda c: c.Co == 24)      # 24 reduction channels in either packing
    for ks in (1, 3, 5):
        for tail in (0, 1):
            assert _has(A, lambda c: c.KS == ks and _dgrad(c).tail == tail), (ks, tail)
    for ks in (1, 3, 5):          # a padded channel row with another image behind it (test_padded_channel_rows_are_not_read)
        assert _has(A, lambda c: c.KS == ks and c.Ci & 15 and c.B > 1), ks
    # images thinner than the filter
    assert _has(A, lambda c: c.H == 1) and _has(A, lambda c: c.W == 1) and _has(A, lambda c: c.W == 2 and c.KS == 5)
    assert {c.KS for _, c in cc.cases(A) if c.up2 and (c.H, c.W) == (2, 2)} == {1, 3, 5}       # a 1x1 source
    assert _has(A, lambda c: c.up2 and (c.H, c.W) == (6, 10) and c.KS == 3)     # odd source sizes: 3 x 5
    assert _has(A, lambda c: c.up2 and (c.H, c.W) == (6, 10) and c.KS == 5)


def test_table_b_reaches_every_instance():
    reached = {(g.KS, g.up2, g.CB, g.BM) for g in (_wgrad(c) for _, c in cc.cases("B"))}
    assert reached == set(itertools.product((1, 3, 5), (0, 1), (4, 16, 32, 64, 128), (32, 64, 128)))
    assert len(reached) == 90


def test_table_b_edges():
    Bt = "B"
    assert {5, 17, 33, 65, 129, 200, 256} <= {c.Ci for _, c in cc.cases(Bt)}
    assert _has(Bt, lambda c: c.Ci == 200 and _wgrad(c).CB == 128) and _has(Bt, lambda c: c.Ci == 256 and _wgrad(c).CB == 128)
    # the swapped form through both reduce kernels, with and without accumulate; its neighbours
    assert {(g.small_reduce, c.accumulate) for c, g in ((c, _wgrad(c)) for _, c in cc.cases(Bt)) if g.swapped} == \
        set(itertools.product((0, 1), (0, 1)))
    assert {(g.small_reduce, c.accumulate) for c, g in ((c, _wgrad(c)) for _, c in cc.cases(Bt)) if not g.swapped} == \
        set(itertools.product((0, 1), (0, 1)))
    assert {(c.Ci, c.Co) for _, c in cc.cases(Bt) if not c.up2} >= {(4, 4), (5, 4), (4, 5), (5, 5)}
    assert _has(Bt, lambda c: c.Co <= 4 < c.Ci and c.up2 and not _wgrad(c).swapped)
    assert {_wgrad(c).BM for _, c in cc.cases(Bt) if _wgrad(c).swapped} == {32, 64, 128}
    assert {c.KS for _, c in cc.cases(Bt) if _wgrad(c).swapped} == {1, 3, 5}
    # the three pixel-index branches, in both up2 forms
    for up2 in (0, 1):
        assert {(g.w_pow2, g.hw_pow2) for g in (_wgrad(c) for _, c in cc.cases(Bt) if c.up2 == up2)} == {(1, 1), (1, 0), (0, 0)}
    assert _has(Bt, lambda c: (c.H, c.W) == (3, 8)) and _has(Bt, lambda c: (c.H, c.W) == (6, 10))
    assert _has(Bt, lambda c: (c.B * c.H * c.W) % 32)                            # a partial last K tile
    # K slices
    assert _has(Bt, lambda c: _wgrad(c).splits == 1)
    assert _has(Bt, lambda c: 1 < _wgrad(c).splits < 8 and _wgrad(c).ktiles % _wgrad(c).kps)
    assert _has(Bt, lambda c: _wgrad(c).splits > 8 and _wgrad(c).splits % 8 and _wgrad(c).ktiles % _wgrad(c).kps)
    assert _has(Bt, lambda c: _wgrad(c).splits > 8 and _wgrad(c).ktiles % _wgrad(c).kps == 0)
    assert {_wgrad(c).splits % 16 for _, c in cc.cases(Bt) if _wgrad(c).small_reduce} >= {0, 5}
    # tap tails: 25 taps in tiles of 32 / 8 / 4 / 2, one tap in the last tile of KS 3 at CB 64, a single tap of KS 1
    assert {_wgrad(c).CB for _, c in cc.cases(Bt) if c.KS == 5} == {4, 16, 32, 64, 128}
    assert _has(Bt, lambda c: c.KS == 3 and _wgrad(c).CB == 64) and _has(Bt, lambda c: c.KS == 1 and _wgrad(c).CB == 16)


def test_table_c_reaches_every_instance_and_edge():
    reached = set()
    for _, c in cc.cases("C_cout"):       # forward small_cout<KS, Co>, data gradient small_cin<KS, Co, DGRAD>
        reached |= {("cout", c.KS, c.Co, 0), ("cin", c.KS, c.Co, 1)}
    for _, c in cc.cases("C_cin"):        # forward small_cin<KS, Ci>, data gradient small_cout<KS, Ci, DGRAD>
        reached |= {("cin", c.KS, c.Ci, 0), ("cout", c.KS, c.Ci, 1)}
    assert reached == set(itertools.product(("cout", "cin"), (3, 5), (1, 2, 3, 4), (0, 1))) and len(reached) == 32
    sizes = {(5, 3), (16, 16), (17, 33), (16, 40)}
    for table in ("C_cout", "C_cin"):
        assert {(c.H, c.W) for _, c in cc.cases(table)} == sizes, table
        assert {c.bias for _, c in cc.cases(table)} == {0, 1}, table
        for ks in (3, 5):
            assert {(c.H, c.W) for _, c in cc.cases(table) if c.KS == ks} == sizes, (table, ks)
    # small_cout's reduction channels: the 8-channel chunk, its tail, several chunks; forward and data-gradient form
    assert {c.Ci for _, c in cc.cases("C_cout")} >= {1, 7, 8, 9, 20}
    assert {c.Co for _, c in cc.cases("C_cin")} >= {1, 5, 70}                   # (the data gradient's reduction channels)
    assert all(c.Co != c.Ci for _, c in cc.cases("C_cin") if c.Co > 1)          # Cw differs from the template's channels
    # small_cin's output channels
    assert {c.Co for _, c in cc.cases("C_cin")} >= {1, 5, 70} and {c.Ci for _, c in cc.cases("C_cout")} >= {1, 7, 20}


def test_table_d_reaches_every_instance_and_edge():
    lib = _lib()
    fwd, wg = set(), set()
    for _, c in cc.cases("D"):
        for ns in (2, 3):
            fwd.add(cc.split_fwd_instance(c.B, c.Ci, c.H, c.W, c.Co, c.KS, c.up2, ns))
            if lib.itcv_conv2d_bf16s_supported(c.Co, c.Ci, c.KS):          # the data gradient: Co -> Ci, never up2
                fwd.add(cc.split_fwd_instance(c.B, c.Co, c.H, c.W, c.Ci, c.KS, 0, ns))
            if lib.itcv_conv2d_wgrad_bf16s_supported(c.Ci, c.H, c.W, c.Co, c.KS):
                wg.add(cc.split_wgrad_instance(c.B, c.Ci, c.H, c.W, c.Co, c.KS, ns))
    assert fwd == set(itertools.product((1, 3), (2, 3), (64, 128), (0, 1))) and len(fwd) == 16
    assert wg == set(itertools.product((1, 3), (2, 3), (32, 64, 128), (64, 128))) and len(wg) == 24
    # the forward launches alone reach the 16
    assert {cc.split_fwd_instance(*c[:7], ns) for _, c in cc.cases("D") for ns in (2, 3)} == fwd
    for ks in (1, 3):
        assert {c.W for _, c in cc.cases("D") if c.KS == ks} >= {8, 24}, ks
        assert {c.accumulate for _, c in cc.cases("D") if c.KS == ks} == {0, 1}, ks
        assert _has("D", lambda c: c.KS == ks and c.up2 and c.W == 8)


@pytest.mark.parametrize("table", sorted(cc.TABLES))
def test_seeds_are_fixed_and_distinct(table):
    seeds = [cc.seed_of(c) for _, c in cc.cases(table)]
    assert len(set(seeds)) == len(seeds)
    assert cc.seed_of((2, 16, 6, 10, 5, 1, 0, 1, 0)) == cc.seed_of(cc.Case(2, 16, 6, 10, 5, 1, 0, 1, 0)) == 1809328991


def test_reference_is_fp64_autograd():
    """The reference of a small case against sums written out by hand (up2, bias, accumulate)."""
    import torch
    c = cc.Case(1, 2, 4, 4, 3, 3, 1, 1, 1)
    r = cc.reference(c)
    xu = r.x.double().repeat_interleave(2, 2).repeat_interleave(2, 3)
    xp = torch.zeros(1, 2, 6, 6, dtype=torch.float64)
    xp[:, :, 1:5, 1:5] = xu
    y = torch.zeros(1, 3, 4, 4, dtype=torch.float64)
    dw = r.dw0.double().clone()
    for kh in range(3):
        for kw in range(3):
            win = xp[:, :, kh:kh + 4, kw:kw + 4]
            y += torch.einsum("oc,bchw->bohw", r.w.double()[:, :, kh, kw], win)
            dw[:, :, kh, kw] += torch.einsum("bohw,bchw->oc", r.dy.double(), win)
    y += r.b.double()[None, :, None, None]
    assert r.y.dtype == torch.float64 and torch.allclose(r.y, y, rtol=0, atol=1e-13)
    assert torch.allclose(r.dw, dw, rtol=0, atol=1e-12)
    assert r.dxu.shape == (1, 2, 4, 4) and r.dx.shape == (1, 2, 2, 2)
    assert torch.allclose(r.dx, r.dxu.reshape(1, 2, 2, 2, 2, 2).sum((3, 5)), rtol=0, atol=1e-13)
    assert 0 < r.e32["y"] < 1e-6 and 0 < r.e32["dw"] < 1e-6 and cc.bound_of(0.0) == 2.0 ** -22 and cc.bound_of(1.0) == 2e-5
