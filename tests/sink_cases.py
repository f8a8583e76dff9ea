"""Which branch every task of the two fused Adam carriers takes, as a function of the row count P, the live-row count and whether the
leaf's three base addresses (parameter, exp_avg, exp_avg_sq) are all 16-byte aligned -- a model of the launch geometry only, no arithmetic.

  k_preprocess_backward<SINK>   (csrc/preprocess.hip, the block after `if (!SINK) return;`): 256 rows per workgroup, 896 float4 tasks,
                                 task -> leaf by the T0 table, `cnt = max(0, min(4, live * RF - e))`
  sh16_adam_span / k_sh16_backward<SPLIT, SINK>  (csrc/sh.hip): 64 rows per block, a span of live * 45 (features_rest) and live * 3
                                 (DC block) floats in rounds of 256 float4 plus an element-wise tail, the positions three floats per lane

The constants are restated here on purpose (a model that read them from the kernels could not disagree with them); tests/test_sink_cases_cpu.py
ties them to the source text and asserts that the row counts and live-row counts below reach every class, so that the GPU tests built on
them (tests/test_gpu_sink_geometry.py) cannot quietly lose one."""

# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, 2, 3, 5, 40, 63, 64, 65, 255, 256, 257, 258, 259, 515)      # 40: a two-round features_rest span; 64 / 65: three rounds
LIVE_P = 515
LIVE_COUNTS = (-3, 0, 1, 255, 256, 257, 514, 515, 600)                        # values of the active_rows word at P = LIVE_P
UNALIGNED_P = (5, 259, 515)
UNALIGNED_BYTES = (4, 8, 12)

# ---- preprocess sink ----------------------------------------------------------------------------------------------------------------------
PP_ROWS = 256                                                                 # rows per workgroup
PP_TASKS = 896                                                                # EGS_SINK_TASKS: float4 tasks per workgroup
PP_LEAVES = ("xyz", "opacity", "scaling", "rotation", "features_dc")         # EGS_SINK_MEANS3D .. EGS_SINK_SH, the order of the stage
PP_ROW_FLOATS = (3, 1, 3, 4, 3)
PP_TASK_START = (0, 192, 256, 448, 704, 896)
PP_CLASSES = ("vec", "tail1", "tail2", "tail3", "idle", "scalar4")            # per leaf; "dead" is per workgroup

# ---- spherical-harmonics sink -------------------------------------------------------------------------------------------------------------
SH_ROWS = 64                                                                  # rows per block (one wave)
SH_SPANS = (("rest", 45), ("dc", 3))                                          # floats per row
SH_ROUND_F4 = 256                                                             # float4 per round: four per lane


def live_rows(P, active=None):
    """Rows that take the step: min(P, max(*active_rows, 0)), or P without the word."""
    return P if active is None else min(P, max(active, 0))


def pp_workgroup(live, aligned=True):
    """One workgroup of the preprocess sink with `live` (1 .. 256) rows to step -> {leaf: set of classes its tasks take}."""
    assert 0 < live <= PP_ROWS
    out = {}
    for l, leaf in enumerate(PP_LEAVES):
        seen = set()
        for task in range(PP_TASK_START[l], PP_TASK_START[l + 1]):
            e = 4 * (task - PP_TASK_START[l])
            cnt = max(0, min(4, live * PP_ROW_FLOATS[l] - e))
            seen.add("idle" if cnt == 0 else ("vec" if aligned else "scalar4") if cnt == 4 else f"tail{cnt}")
        out[leaf] = seen
    return out


def pp_classes(P, active=None, aligned=True):
    """-> ({leaf: classes reached over all workgroups of a launch over P rows}, number of dead workgroups)."""
    rows, dead = live_rows(P, active), 0
    out = {leaf: set() for leaf in PP_LEAVES}
    for b in range((P + PP_ROWS - 1) // PP_ROWS):
        live = min(PP_ROWS, rows - b * PP_ROWS)
        if live <= 0:
            dead += 1
            continue
        for leaf, seen in pp_workgroup(live, aligned).items():
            out[leaf] |= seen
    return out, dead


def pp_possible(leaf):
    """Every class a task of `leaf` can take at all (any live count, either alignment): a leaf of four floats per row has no tail."""
    seen = set()
    for live in range(1, PP_ROWS + 1):
        for aligned in (True, False):
            seen |= pp_workgroup(live, aligned)[leaf]
    return seen


def sh_block(live, aligned=True):
    """One block of the spherical-harmonics sink with `live` (1 .. 64) rows -> {"rest": ..., "dc": ..., "xyz": ...}: the span classes are
    "rounds<k>" (rounds of the vector loop in which at least one float4 is stepped) and "tail<n % 4>", or "scalar-all"."""
    assert 0 < live <= SH_ROWS
    out = {}
    for name, per_row in SH_SPANS:
        n = live * per_row
        if aligned:
            n4 = n // 4
            out[name] = {f"rounds{(n4 + SH_ROUND_F4 - 1) // SH_ROUND_F4}", f"tail{n % 4}"}
        else:
            out[name] = {"scalar-all"}
    out["xyz"] = {"lanes64" if live == SH_ROWS else "lanes<64"}
    return out


def sh_classes(P, active=None, aligned=True):
    """-> ({"rest" / "dc" / "xyz": classes reached over all blocks of a launch over P rows}, number of dead blocks)."""
    rows, dead = live_rows(P, active), 0
    out = {"rest": set(), "dc": set(), "xyz": set()}
    for b in range((P + SH_ROWS - 1) // SH_ROWS):
        live = min(SH_ROWS, rows - b * SH_ROWS)
        if live <= 0:
            dead += 1
            continue
        for name, seen in sh_block(live, aligned).items():
            out[name] |= seen
    return out, dead


def sh_possible(name):
    seen = set()
    for live in range(1, SH_ROWS + 1):
        for aligned in (True, False):
            seen |= sh_block(live, aligned)[name]
    return seen


def describe(P, active=None, aligned=True):
    """One line for a log: the classes a case reaches in both kernels."""
    pp, pp_dead = pp_classes(P, active, aligned)
    sh, sh_dead = sh_classes(P, active, aligned)
    fmt = lambda d: "; ".join(f"{k}: {' '.join(sorted(v)) or '-'}" for k, v in d.items())
    return f"P={P} active={active} aligned={aligned} | preprocess [{fmt(pp)}] dead workgroups {pp_dead} | sh [{fmt(sh)}] dead blocks {sh_dead}"
