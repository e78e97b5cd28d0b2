"""cc_logits_penalize_streams / cc_logits_constrain_streams without a device: the two symbols are in the header and in _abi.py with
matching argument counts and record layouts, device-only and exported, and every refusal comes before any launch (this machine has
no device: a launch would fail with another code)."""
import ctypes as C

from logits_rows_common import _check_refusals


def test_the_refusals_come_before_any_launch():
    """the same calls on host memory, on a machine without a device: a launch would fail with another code (or fault)"""
    _check_refusals("cpu")


def test_abi_surface():
    import os
    import re

    from cold_compress_amd import _abi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "coldcompress.h")).read()
    for name in ("cc_logits_penalize_streams", "cc_logits_constrain_streams"):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == len(_abi.SIGNATURES[name][1]) == 10, name
        assert name in _abi.DEVICE_ONLY
    # the records' layout is the header's: natural alignment, pointers first where the header has them first
    assert C.sizeof(_abi.PenaltyRow) == 48 and _abi.PenaltyRow.r.offset == 32 and _abi.PenaltyRow.p.offset == 40
    assert C.sizeof(_abi.ConstraintRow) == 80 and _abi.ConstraintRow.gen_start.offset == 16 and _abi.ConstraintRow.term_ids.offset == 40
    assert _abi.ConstraintRow.bw_tokens.offset == 56 and _abi.ConstraintRow.n_bw.offset == 72


def test_the_constraint_cases_make_every_rule_bite():
    """the histories of the device comparison are built so that every rule bans at least one element in at least one row"""
    from logits_rows_common import RULE_NAMES, con_hits

    for cap in (64, 3000):
        hits = con_hits(cap)
        assert set(hits) == RULE_NAMES and all(n > 0 for n in hits.values()), (cap, hits)
