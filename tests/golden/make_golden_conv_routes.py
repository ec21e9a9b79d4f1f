"""Writes tests/golden/conv_routes.json: what the separate conv routing predicates of hipvae/functional.py answered
before they were folded into one route record (``conv_route``).  It ran at the last commit that still had them
(``_planes_ns``, ``_dgrad_sub_kind``, ``_wgrad5_mode``, ``_wgrad_planes_ok``, ``conv_input_mode``, ``conv_grad_mode``,
``conv_input_planes_ns``, ``conv_grad_planes_ns``) and does not run on a later tree; it is kept as the record of how the
table was made.  Host queries only: the cross-compiled library is enough, no GPU.

    python tests/golden/make_golden_conv_routes.py

Layout: ``cases`` = [B, Ci, H, W, Co, KS, up2, [row index per variant]] with the variants in the order of
``test_conv_route_host.VARIANTS``; ``rows`` = the distinct answers, columns as in ``COLUMNS``; ``mixed`` = [shape,
forward mode, backward mode, weight gradient misses fp32 x, data gradient misses its sub-range form]: the two
conditions under which Conv2dFn.backward raises "conv math mode changed ..."."""
import json
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "intro-tc-vae_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)
import test_conv_route_host as T  # noqa: E402
from hipvae import functional as HF  # noqa: E402


def answers(B, Ci, H, W, Co, KS, up2, nig, bias):
    conv = SimpleNamespace(in_channels=Ci, out_channels=Co, kernel_size=(KS, KS), bias=object() if bias else None)
    ns = HF._planes_ns(Ci, Co, KS, up2)
    wg_ok = HF._wgrad_planes_ok(B, Ci, H, W, Co, KS)
    wg5 = HF._wgrad5_mode(Ci, H, W, Co, KS, up2)
    keep_xp = bool(HF._two(ns) and (wg_ok or wg5 == "predict"))          # Conv2dFn.forward
    return [ns, HF._planes_ns(Co, Ci, KS, False), HF._dgrad_sub_kind(Co, Ci, KS), wg5, wg_ok,
            list(HF.conv_input_mode(conv, B, H, W, up2)), list(HF.conv_grad_mode(conv, B, H, W, nig)),
            HF.conv_input_planes_ns(conv, up2), HF.conv_grad_planes_ns(conv, nig), keep_xp]


def mixed(shape, fmode, bmode):
    """Conv2dFn.forward in ``fmode``, Conv2dFn.backward (all three gradients wanted) in ``bmode``."""
    B, Ci, H, W, Co, KS, up2 = shape
    with HF.conv_math_scope(fmode):
        ns = HF._planes_ns(Ci, Co, KS, up2)
        x_saved = not (HF._two(ns) and (HF._wgrad_planes_ok(B, Ci, H, W, Co, KS)
                                        or HF._wgrad5_mode(Ci, H, W, Co, KS, up2) == "predict"))
        live_possible = HF._dgrad_sub_kind(Co, Ci, KS) is not None       # else the forward blocks the live range
    with HF.conv_math_scope(bmode):
        fmt2 = HF.F16X2 if HF._NS[bmode] == HF.F16X2 else 2
        raw = (HF._wgrad5_mode(Ci, H, W, Co, KS, up2) is None
               and not (HF._wgrad_planes_ok(B, Ci, H, W, Co, KS) and HF._planes_ns(Co, Ci, KS, False) in (0, fmt2)))
        sub_gone = HF._dgrad_sub_kind(Co, Ci, KS) is None
    return [list(shape), fmode, bmode, bool(raw and not x_saved), bool(live_possible and sub_gone)]


def main():
    rows, index, cases = [], {}, []
    for shape in T.shapes():
        idx = []
        for mode, scin, nig, bias in T.VARIANTS:
            HF._SCIN_MFMA[0] = scin
            with HF.conv_math_scope(mode):
                a = answers(*shape[:6], bool(shape[6]), nig, bias)
            k = json.dumps(a)
            if k not in index:
                index[k] = len(rows)
                rows.append(a)
            idx.append(index[k])
        cases.append(list(shape) + [idx])
    HF._SCIN_MFMA[0] = True
    out = {"columns": list(T.COLUMNS), "variants": [list(v) for v in T.VARIANTS], "rows": rows, "cases": cases,
           "mixed": [mixed(s, f, b) for s in T.MIXED_SHAPES for f, b in T.MIXED_PAIRS]}
    path = os.path.join(HERE, "conv_routes.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()) + "\n}\n")
    print(path, len(cases), "cases", len(rows), "distinct rows", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
