"""scripts/check_isa.py's held-M0 rule (the render kernels' weight DMA: piece 0 of a chunk writes M0,
pieces 1-3 reuse it) on toy instruction lists: what the rule accepts and what it must reject."""
import os
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "scripts"))
import check_isa   # noqa: E402

PIECE0 = ["s_mov_b32 m0, s20", "s_nop 0", "global_load_lds_dwordx4 v1, s[2:3]"]
PIECE = "global_load_lds_dwordx4 v1, s[2:3] offset:1024"
MFMA = "v_mfma_f32_16x16x32_f16 a[0:3], v[0:3], v[4:7], a[0:3]"
SAVED = ["s_mov_b32 s9, m0", "s_mov_b32 m0, s8", "s_nop 0", "global_load_lds_dwordx4 v2, s[4:5]", "s_mov_b32 m0, s9"]


def listing(lines, branch_to=None):
    """[(address, instruction, branch target)]; `branch_to` = (index of a branch line, index of its target)."""
    out = []
    for i, ins in enumerate(lines):
        tgt = 4 * branch_to[1] if branch_to and i == branch_to[0] else None
        out.append((4 * i, ins, tgt))
    return out


def test_chunk_pattern_is_accepted():
    lines = PIECE0 + [MFMA, PIECE, MFMA, MFMA, PIECE, MFMA, PIECE, "s_waitcnt vmcnt(4)", "s_barrier"] + PIECE0 + [PIECE]
    assert check_isa.check_held_m0(listing(lines)) == []


def test_saved_piece_between_keeps_the_held_value():
    lines = PIECE0 + [MFMA] + SAVED + [PIECE]
    assert check_isa.check_held_m0(listing(lines)) == []
    # a saved piece restores what it found: nothing held before it, nothing held after it
    assert check_isa.check_held_m0(listing([MFMA] + SAVED + [PIECE]))


@pytest.mark.parametrize("between", [["s_barrier"], ["s_endpgm"], ["s_mov_b32 m0, s7"], ["s_cbranch_scc1 0"]])
def test_piece_without_a_held_m0_is_rejected(between):
    assert check_isa.check_held_m0(listing(PIECE0 + [MFMA] + between + [MFMA, PIECE]))


def test_piece_with_no_m0_write_before_it_is_rejected():
    assert check_isa.check_held_m0(listing([MFMA, PIECE]))


def test_branch_target_between_is_rejected():
    lines = PIECE0 + [MFMA, MFMA, PIECE, "s_cbranch_scc1 back"]
    assert check_isa.check_held_m0(listing(lines, branch_to=(6, 4)))       # the loop re-enters between pieces
    assert check_isa.check_held_m0(listing(lines, branch_to=(6, 0))) == []  # re-entering at piece 0 is fine


def test_other_kernels_keep_the_strict_rule():
    insns = PIECE0 + [MFMA, PIECE]
    bad, pieces = check_isa.check_function(insns)
    assert pieces == 1 and any("not directly behind" in b for b in bad)
    bad, pieces = check_isa.check_function(insns, hold=True)
    assert pieces == 2 and bad == []
