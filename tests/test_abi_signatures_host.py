"""CPU-only checks of the derived binding: hipvae.abi builds its ctypes table and its integer constants from
include/itcv_hip.h.  The table equals the hand-written one it replaced (tests/golden/abi_v4_signatures.json, recorded
from that commit's source), the constants keep their values, the parser maps a closed set of C types and refuses the
rest, and the one device check says its one sentence."""
import ctypes
import json
import os

import pytest
import torch

from hipvae import abi
from hipvae import functional as HF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = {"p": ctypes.c_void_p, "i32": ctypes.c_int, "i64": ctypes.c_int64, "sz": ctypes.c_size_t,
         "f32": ctypes.c_float, "f64": ctypes.c_double, "cp": ctypes.c_char_p}
SENTENCE = "HIP kernels need device tensors (got a CPU tensor); there is no CPU path"


def test_derived_table_equals_the_hand_table_it_replaced():
    with open(os.path.join(ROOT, "tests", "golden", "abi_v4_signatures.json")) as f:
        fixture = json.load(f)
    assert len(fixture["parent"]) == 40
    hand = fixture["signatures"]
    assert len(hand) == 193
    for name, (res, args) in hand.items():
        assert name in abi.SIGNATURES, name
        got_res, got_args = abi.SIGNATURES[name]
        assert got_res is SHORT[res], (name, got_res, res)
        assert len(got_args) == len(args), (name, len(got_args), len(args))
        for k, (g, a) in enumerate(zip(got_args, args)):
            assert g is SHORT[a], (name, k, g, a)
    with open(abi.HEADER) as f:
        header = f.read()
    for name in abi.SIGNATURES:
        assert name + "(" in header, f"{name} is in the table but not in the header"


def test_constants_keep_their_values():
    assert abi.ABI_VERSION == 4
    assert (abi.TC_VAR_FROM_ROW, abi.TC_EPS_DENSITY, abi.TC_WEIGHTED, abi.TC_LIVE) == (1, 2, 4, 3)
    assert (abi.OPT_MAXIMIZE, abi.OPT_NESTEROV, abi.OPT_AMSGRAD, abi.OPT_DECOUPLED_WD, abi.OPT_CENTERED) == (
        0x1, 0x2, 0x4, 0x8, 0x10)
    assert abi.LOSS_TYPES == {"mse": 0, "l1": 1, "bce": 2}
    assert abi.BN_PATHS == ("OneBlock", "SlicedFold", "SlicedCombine", "Fallback", "PerGroup", "TileStats")
    assert HF.F16X2 == 4
    assert HF.GBT_NODES == 127
    for v in (abi.ABI_VERSION, abi.TC_LIVE, abi.OPT_CENTERED, HF.F16X2, HF.GBT_NODES):
        assert type(v) is int


def test_parser_prototypes():
    sig, _ = abi.parse_header("""
        #include <stddef.h>
        extern "C" {
        int itcv_a(void);
        size_t itcv_b();
        int itcv_spread(const float* x,
                        size_t n,   // trailing comment, with a comma
                        double eps,
                        void* stream);
        /* int itcv_in_block(int n);
           int itcv_in_block_too(int n); */
        // int itcv_after_slashes(int n);
        int itcv_ptrs(const float* const* rows, uint8_t* out, const void *ws, char** names);
        const char* itcv_text(const char* name, const char *other);
        int itcv_wide(long long a, int64_t b, const int64_t c, long long, float f, int);
        }
    """)
    assert sorted(sig) == ["itcv_a", "itcv_b", "itcv_ptrs", "itcv_spread", "itcv_text", "itcv_wide"]
    assert sig["itcv_a"] == (ctypes.c_int, [])
    assert sig["itcv_b"] == (ctypes.c_size_t, [])
    assert sig["itcv_spread"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_void_p])
    assert sig["itcv_ptrs"] == (ctypes.c_int, [ctypes.c_void_p] * 4)
    assert sig["itcv_text"] == (ctypes.c_char_p, [ctypes.c_char_p, ctypes.c_char_p])
    assert sig["itcv_wide"] == (ctypes.c_int, [ctypes.c_int64] * 4 + [ctypes.c_float, ctypes.c_int])


@pytest.mark.parametrize("params, named", [
    ("unsigned n", "unsigned n"),
    ("struct Foo f", "struct Foo f"),
    ("int n, void (*done)(int, void*)", "function-pointer"),
    ("int n, foo_t", "foo_t"),
    ("int n, long m", "long m"),
    ("int n,", "''"),
])
def test_parser_refuses_what_it_cannot_map(params, named):
    with pytest.raises(abi.HipExtensionError) as e:
        abi.parse_header(f"int itcv_good(int n);\nint itcv_bad({params});\n")
    assert "itcv_bad" in str(e.value) and named in str(e.value)


def test_parser_refuses_an_unknown_return_type():
    with pytest.raises(abi.HipExtensionError, match="itcv_bad.*unsigned"):
        abi.parse_header("unsigned itcv_bad(int n);")
    with pytest.raises(abi.HipExtensionError, match="itcv_nothing.*void"):
        abi.parse_header("void itcv_nothing(int n);")


def test_parser_defines():
    _, d = abi.parse_header("""
        #ifndef ITCV_GUARD_H
        #define ITCV_GUARD_H
        #define ITCV_ONE 0x1   /* a comment */
        #define ITCV_FOUR 4    // another
        # define ITCV_BOTH (ITCV_ONE | ITCV_FOUR)
        #define ITCV_BUDGET ((size_t)512 << 20)
        #define ITCV_SHIFT (1 << 3)
        #define ITCV_EARLY (ITCV_ONE | ITCV_LATER)
        #define ITCV_LATER 8
        #define ITCV_NAME "text"
        // #define ITCV_COMMENTED 9
        #define OTHER_THING 3
        #endif
    """)
    assert d == {"ITCV_ONE": 1, "ITCV_FOUR": 4, "ITCV_BOTH": 5, "ITCV_LATER": 8}


def test_need_device():
    with pytest.raises(abi.HipExtensionError) as e:
        abi.need_device(torch.zeros(2))
    assert str(e.value) == SENTENCE
    abi.need_device()
    abi.need_device(None, None)
    with pytest.raises(abi.HipExtensionError) as e:
        abi.need_device(None, torch.zeros(2, 3), None)
    assert str(e.value) == SENTENCE
    with pytest.raises(abi.HipExtensionError) as e:
        abi.ptr(torch.zeros(2))
    assert str(e.value) == SENTENCE
    assert abi.ptr(None) is None


def test_the_sentence_is_written_once():
    pkg = os.path.join(ROOT, "intro-tc-vae_amd")
    files = [os.path.join(pkg, "ops.py")] + sorted(
        os.path.join(pkg, "hipvae", f) for f in os.listdir(os.path.join(pkg, "hipvae")) if f.endswith(".py"))
    hits = {}
    for path in files:
        with open(path) as f:
            n = f.read().count("got a CPU tensor")
        if n:
            hits[os.path.relpath(path, pkg)] = n
    assert hits == {os.path.join("hipvae", "abi.py"): 1}, hits
    with open(os.path.join(pkg, "hipvae", "abi.py")) as f:
        assert f.read().count(SENTENCE) == 1
