"""CPU: the case lists of tests/test_gpu_sink_geometry.py reach every branch class of the two fused Adam carriers (tests/sink_cases.py).
A condition on the inputs, not a measurement: a later change of a list that loses a class fails here, on a machine without a GPU."""
import os
import re

from tests import sink_cases as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "egogaussian_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_model_constants_are_the_kernels():
    common = _text("egs_common.h")
    assert re.search(r"^#define\s+EGS_SINK_TASKS\s+896\b", common, re.M) and S.PP_TASKS == 896
    assert re.search(r"^#define\s+EGS_SINK_PP_LEAVES\s+5\b", common, re.M) and len(S.PP_LEAVES) == len(S.PP_ROW_FLOATS) == 5
    pp = _text("preprocess.hip")
    assert "RF[EGS_SINK_PP_LEAVES] = { " + ", ".join(map(str, S.PP_ROW_FLOATS)) + " }" in pp
    assert "T0[EGS_SINK_PP_LEAVES + 1] = { " + ", ".join(map(str, S.PP_TASK_START)) + " }" in pp
    assert "const int row0 = blockIdx.x * 256;" in pp and S.PP_ROWS == 256
    sh = _text("sh.hip")
    assert "(size_t)i0 * 45, live * 45" in sh and "(size_t)i0 * 3, live * 3" in sh and dict(S.SH_SPANS) == {"rest": 45, "dc": 3}
    assert "const int live = min(64, rows - i0);" in sh and S.SH_ROWS == 64
    assert "q0 += 4 * 64" in sh and S.SH_ROUND_F4 == 4 * 64
    # the table itself: every leaf owns 64 * row floats tasks (256 rows * row floats / 4), back to back
    assert S.PP_TASK_START[0] == 0 and S.PP_TASK_START[-1] == S.PP_TASKS
    for l, rf in enumerate(S.PP_ROW_FLOATS):
        assert S.PP_TASK_START[l + 1] - S.PP_TASK_START[l] == S.PP_ROWS * rf // 4


def test_model_on_cases_worked_by_hand():
    full = S.pp_workgroup(256)
    assert all(full[leaf] == {"vec"} for leaf in S.PP_LEAVES)                   # a full workgroup: 896 vector tasks, nothing idle
    one = S.pp_workgroup(1)
    assert one["xyz"] == one["scaling"] == one["features_dc"] == {"tail3", "idle"}
    assert one["opacity"] == {"tail1", "idle"} and one["rotation"] == {"vec", "idle"}
    assert S.pp_workgroup(1, aligned=False)["rotation"] == {"scalar4", "idle"}
    assert S.pp_workgroup(3)["xyz"] == {"vec", "vec", "tail1", "idle"}          # 9 floats: two float4 and one element
    assert S.pp_classes(515, active=256)[1] == 2 and S.pp_classes(515, active=-3)[1] == 3 and S.pp_classes(515, active=600)[1] == 0
    assert S.sh_block(64) == {"rest": {"rounds3", "tail0"}, "dc": {"rounds1", "tail0"}, "xyz": {"lanes64"}}       # 720 and 48 float4
    assert S.sh_block(40)["rest"] == {"rounds2", "tail0"}                                                          # 450 float4
    assert S.sh_block(1) == {"rest": {"rounds1", "tail1"}, "dc": {"rounds0", "tail3"}, "xyz": {"lanes<64"}}       # 11 float4 + 1; 3 floats
    assert S.sh_block(22)["rest"] == {"rounds1", "tail2"} and S.sh_block(23)["rest"] == {"rounds2", "tail3"}      # 247 | 258 float4
    assert S.sh_block(5, aligned=False)["rest"] == S.sh_block(5, aligned=False)["dc"] == {"scalar-all"}
    assert S.sh_classes(515, active=257)[1] == 4 and S.sh_classes(515, active=0)[1] == 9


def test_what_each_leaf_can_reach_at_all():
    tails = {"tail1", "tail2", "tail3"}
    for leaf, rf in zip(S.PP_LEAVES, S.PP_ROW_FLOATS):
        want = {"vec", "scalar4", "idle"} | (set() if rf == 4 else tails)      # four floats per row: live * 4 is never 1 .. 3 past a task start
        assert S.pp_possible(leaf) == want, leaf
    assert not S.pp_possible("rotation") & tails
    assert S.sh_possible("rest") == {"rounds1", "rounds2", "rounds3", "tail0", "tail1", "tail2", "tail3", "scalar-all"}    # at least 11 float4
    assert S.sh_possible("dc") == {"rounds0", "rounds1", "tail0", "tail1", "tail2", "tail3", "scalar-all"}                 # at most 48 float4
    assert S.sh_possible("xyz") == {"lanes64", "lanes<64"}


def _union(cases, fn):
    out, dead = {}, 0
    for kw in cases:
        got, d = fn(**kw)
        dead += d
        for k, v in got.items():
            out.setdefault(k, set()).update(v)
    return out, dead


def test_row_counts_reach_every_aligned_class_and_no_dead_workgroup():
    cases = [dict(P=P) for P in S.ROW_COUNTS]
    pp, dead = _union(cases, S.pp_classes)
    assert dead == 0
    for leaf in S.PP_LEAVES:
        assert pp[leaf] == S.pp_possible(leaf) - {"scalar4"}, leaf
    sh, dead = _union(cases, S.sh_classes)
    assert dead == 0
    for name in ("rest", "dc", "xyz"):
        assert sh[name] == S.sh_possible(name) - {"scalar-all"}, name
    # the row counts the issue names for a reason
    assert "rounds2" in S.sh_classes(40)[0]["rest"] and "rounds3" in S.sh_classes(64)[0]["rest"] and "rounds3" in S.sh_classes(65)[0]["rest"]
    assert max(S.ROW_COUNTS) > 2 * S.PP_ROWS and any(P >= 255 for P in S.ROW_COUNTS)


def test_live_counts_reach_dead_workgroups_and_every_tail():
    cases = [dict(P=S.LIVE_P, active=a) for a in S.LIVE_COUNTS]
    for a in S.LIVE_COUNTS:
        blocks = (S.LIVE_P + S.PP_ROWS - 1) // S.PP_ROWS
        want_dead = blocks - (S.live_rows(S.LIVE_P, a) + S.PP_ROWS - 1) // S.PP_ROWS
        assert S.pp_classes(S.LIVE_P, a)[1] == want_dead
    assert S.pp_classes(S.LIVE_P, -3)[1] == S.pp_classes(S.LIVE_P, 0)[1] == 3 and S.sh_classes(S.LIVE_P, 0)[1] == 9        # every workgroup dead
    assert S.pp_classes(S.LIVE_P, 256)[1] == 2 and S.pp_classes(S.LIVE_P, 257)[1] == 1                                      # the edge itself
    assert S.pp_classes(S.LIVE_P, 600) == S.pp_classes(S.LIVE_P, 515) == S.pp_classes(S.LIVE_P)                             # clamped to P
    pp, dead = _union(cases, S.pp_classes)
    assert dead > 0
    for leaf in S.PP_LEAVES:
        assert pp[leaf] == S.pp_possible(leaf) - {"scalar4"}, leaf
    sh, dead = _union(cases, S.sh_classes)
    assert dead > 0
    for name in ("rest", "dc"):
        assert {"tail0", "tail1", "tail2", "tail3"} <= sh[name], name
    assert sh["xyz"] == {"lanes64", "lanes<64"}


def test_unaligned_cases_reach_the_scalar_classes_with_tails_beside_them():
    cases = [dict(P=P, aligned=False) for P in S.UNALIGNED_P]
    pp, _ = _union(cases, S.pp_classes)
    for leaf, rf in zip(S.PP_LEAVES, S.PP_ROW_FLOATS):                        # full tasks element by element, beside tails and idle tasks
        assert {"scalar4", "idle"} <= pp[leaf] and "vec" not in pp[leaf], leaf
        assert rf == 4 or {"tail1", "tail3"} <= pp[leaf], leaf
    sh, _ = _union(cases, S.sh_classes)
    assert sh["rest"] == sh["dc"] == {"scalar-all"}
    assert set(S.UNALIGNED_BYTES) == {4, 8, 12}
