"""CPU-only: the ``stream_nt`` option (include/itcv_hip.h, abi.hip).  It is a mask with one bit per kernel family; the
library starts with ITCV_STREAM_NT_DEFAULT, takes any value >= 0, keeps the bits of ITCV_STREAM_NT_ALL and hands them
back; ``hipvae/abi.py`` reads the bits and the two masks from the header; DESIGN.md section 4 states the default."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"BN_APPLY": 0x1, "WGRAD_SLABS": 0x2, "FOLD": 0x4, "WGRAD_OPS": 0x8, "OPTIM": 0x10, "BN_FWD": 0x20}


@pytest.fixture()
def HF():
    from hipvae import functional
    prev = functional.get_option("stream_nt")
    yield functional
    functional.set_option("stream_nt", prev)


def test_bits_and_masks_come_from_the_header():
    from hipvae import abi
    text = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lits = {k: int(v, 16) for k, v in re.findall(r"#define ITCV_STREAM_NT_([A-Z_]+) (0x[0-9a-fA-F]+)\b", text)}
    assert lits == FAMILIES
    assert {k: v for k, v in abi.STREAM_NT.items() if k not in ("ALL", "DEFAULT")} == FAMILIES
    assert abi.STREAM_NT["ALL"] == 0x3F
    assert abi.STREAM_NT["DEFAULT"] & ~abi.STREAM_NT["ALL"] == 0
    assert abi.STREAM_NT["DEFAULT"] & (FAMILIES["WGRAD_OPS"] | FAMILIES["OPTIM"]) == 0     # reserved: no kernel reads them
    # abi.py holds no literal of its own
    src = open(os.path.join(ROOT, "intro-tc-vae_amd", "hipvae", "abi.py")).read()
    assert '_defs("ITCV_STREAM_NT_")' in src and not re.search(r"STREAM_NT\w*\s*=\s*(0x|\d)", src)


def test_default_is_the_header_mask_and_what_design_states(HF):
    from hipvae import abi
    # the library starts with the header's mask (every test that sets the option puts the previous value back)
    assert "int g_stream_nt = ITCV_STREAM_NT_DEFAULT;" in open(os.path.join(abi.CSRC, "abi.hip")).read()
    assert HF.get_option("stream_nt") == abi.STREAM_NT["DEFAULT"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"`stream_nt` default: `(0x[0-9a-fA-F]+)` = ([A-Z_ |]+)\n", design)
    assert m, "DESIGN.md section 4 states the default mask as: `stream_nt` default: `0x..` = NAME | NAME"
    assert int(m.group(1), 16) == abi.STREAM_NT["DEFAULT"]
    named = 0
    for name in m.group(2).split("|"):
        named |= FAMILIES[name.strip()]
    assert named == abi.STREAM_NT["DEFAULT"]


def test_accepted_clamped_and_read_back(HF):
    from hipvae import abi
    ALL = abi.STREAM_NT["ALL"]
    for value in (0, 1, 0x15, ALL):
        HF.set_option("stream_nt", value)
        assert HF.get_option("stream_nt") == value
    for value, kept in ((ALL + 1, 0), (0x7FFFFFFF, ALL), (0x140 | 0x4, 0x4)):
        HF.set_option("stream_nt", value)                  # bits outside the mask are dropped, not refused
        assert HF.get_option("stream_nt") == kept
    HF.set_option("stream_nt", 0x21)
    for bad in (-1, -0x40):
        with pytest.raises(abi.HipExtensionError, match="stream_nt"):
            HF.set_option("stream_nt", bad)
        assert HF.get_option("stream_nt") == 0x21          # a refused value changes nothing
    with HF.option_scope("stream_nt", 0x2):
        assert HF.get_option("stream_nt") == 0x2
    assert HF.get_option("stream_nt") == 0x21
