"""CPU: the host half of the JPEG reader (egogaussian_amd/jpeg.py): decode() -- the statement the kernels of csrc/jpeg_decode.hip answer to --
against the pixels Pillow gave for the golden files, byte for byte; the refusals of parse(); plan(); the range rule."""
import re

import numpy as np
import pytest

from tests import jpeg_cases as JC


def test_the_golden_archive_holds_what_the_issue_lists():
    g = JC.golden()
    for size in ("1x1", "8x8", "9x17", "16x16", "17x33", "31x15", "37x53"):
        for variant in ("444", "422", "420", "L"):
            assert f"{size}-{variant}" in g
    assert {"37x53-420-rb1", "37x53-420-rb2", "37x53-444-rr1", "72x72-444-rb1", "72x72-444", "16x16-420-app1-com"} <= set(g)
    assert all(b"\xff\x00" in g[f"24x40-{s}-q100-noise"][0] for s in ("444", "422", "420"))
    for name, (data, pixels) in g.items():
        w, h = (int(v) for v in name.split("-")[0].split("x"))
        assert pixels.shape == (h, w, 1 if "-L" in name else 3) and pixels.dtype == np.uint8, name


@pytest.mark.parametrize("name", list(JC.golden()))
def test_decode_equals_pillow_byte_for_byte(name):
    from egogaussian_amd import jpeg
    data, pixels = JC.golden()[name]
    got = jpeg.decode(data)
    assert got.dtype == np.uint8 and got.shape == pixels.shape
    assert np.array_equal(got, pixels), f"{name}: {int((got != pixels).sum())} bytes differ"


def test_the_fixtures_exercise_what_they_are_there_for():
    from egogaussian_amd import jpeg
    g = JC.golden()
    p = jpeg.parse(g["37x53-420-rb1"][0])
    assert jpeg.geometry(p) == (3, 4, 6, 12) and p["restart_interval"] == 1, "12 intervals: the marker number wraps"
    assert jpeg.geometry(jpeg.parse(g["72x72-444-rb1"][0]))[3] == 81, "more intervals than a wave has lanes"
    assert jpeg.geometry(jpeg.parse(g["37x53-444-rr1"][0]))[3] == 7
    assert jpeg.parse(g["17x33-420"][0])["hs"] == 2 and 17 % 16 == 1, "the chroma edge at a column that is no MCU edge"
    lengths = jpeg.parse(g["37x53-444-opt30"][0])["ac"][0][0]
    assert lengths[8:].any(), "optimised tables with codes longer than the first-level look-up"
    assert jpeg.parse(g["4x3-420"][0])["W"] == 4 and jpeg.parse(g["5x6-420"][0])["W"] == 5, "chroma planes of two and of three columns"
    twin_a, twin_b = g["72x72-444-rb1"], g["72x72-444"]
    assert twin_a[0] != twin_b[0] and np.array_equal(twin_a[1], twin_b[1])
    assert np.array_equal(jpeg.decode(twin_a[0]), jpeg.decode(twin_b[0]))


@pytest.mark.parametrize("wrong", ["nearest-neighbour chroma", "the rounding constants swapped", "the MCU-padded width for the last-column rule",
                                   "the row pass before the column pass", ">> 16 without the half", "no DC reset at a restart"])
def test_the_fixtures_tell_a_wrong_statement_apart(wrong):
    """A statement that differs from decode() in one point differs from Pillow's pixels on some fixture."""
    from egogaussian_amd import jpeg
    assert wrong in jpeg.WRONG
    differing = [n for n, (data, pixels) in JC.golden().items() if not np.array_equal(jpeg.decode(data, wrong=wrong), pixels)]
    assert differing, wrong


@pytest.mark.parametrize("name", list(JC.refusals()))
def test_parse_refuses_by_name(name):
    from egogaussian_amd import jpeg
    data, words = JC.refusals()[name]
    with pytest.raises(ValueError, match=words) as e:
        jpeg.parse(data)
    assert str(e.value).startswith("jpeg.parse: ") and not isinstance(e.value, jpeg.StatusError)


def test_parse_advice_and_the_fields_it_returns():
    from egogaussian_amd import jpeg
    from egogaussian_amd.ingest import _ADVICE
    for name in ("SOF2", "12-bit samples", "16-bit quantisation table", "four components", "a scan of one component", "luma 1x2",
                 "Adobe transform 0 without JFIF"):
        with pytest.raises(ValueError, match=re.escape(_ADVICE)):
            jpeg.parse(JC.refusals()[name][0])
    data = JC.golden()["16x16-420-app1-com"][0]
    p = jpeg.parse(data)
    assert (p["W"], p["H"], p["C"], p["hs"], p["vs"], p["restart_interval"]) == (16, 16, 3, 2, 2, 0)
    assert data[p["entropy_begin"] - 14:p["entropy_begin"] - 12] == b"\xff\xda" and p["quant"].shape == (4, 64)
    assert p["tq"] == [0, 1, 1] and p["td"] == [0, 1, 1] and p["ta"] == [0, 1, 1]
    assert p["quant"][0][1] == data[data.index(b"\xff\xdb") + 6], "natural order: entries 0 and 1 are the first two in zigzag order too"
    assert p["quant"][0][8] == data[data.index(b"\xff\xdb") + 7], "... and entry 8 is the third"
    grey = jpeg.parse(JC.golden()["31x15-L-rb2"][0])
    assert (grey["C"], grey["hs"], grey["vs"], grey["restart_interval"]) == (1, 1, 1, 2) and jpeg.geometry(grey) == (4, 2, 1, 4)


def test_plan_arithmetic_and_alignments():
    from egogaussian_amd import jpeg
    names = ["37x53-420-rb1", "1x1-L", "17x33-422", "9x17-444"]
    parsed = [dict(jpeg.parse(JC.golden()[n][0]), nbytes=len(JC.golden()[n][0])) for n in names]
    p = jpeg.plan(parsed, out_gap=256)
    d = p["desc"]
    assert d.dtype.itemsize == 104 and p["tables"].dtype.itemsize == 2432
    assert d["n_intervals"].tolist() == [12, 1, 1, 1] and d["interval_begin"].tolist() == [0, 12, 13, 14] and p["n_intervals"] == 15
    assert d["mcus_x"].tolist() == [3, 1, 2, 2] and d["mcus_y"].tolist() == [4, 1, 5, 3]
    blocks = [3 * 4 * 6, 1, 2 * 5 * 4, 2 * 3 * 3]
    up = lambda v, a: -(-v // a) * a
    for k, (name, arr, unit) in enumerate((("file_offset", [x["nbytes"] for x in parsed], 16), ("coef_offset", [128 * b for b in blocks], 16),
                                           ("plane_offset", [64 * b for b in blocks], 16),
                                           ("out_offset", [x["W"] * x["H"] * x["C"] + 256 for x in parsed], 256))):
        at = 0
        for i, size in enumerate(arr):
            assert int(d[name][i]) == at and at % unit == 0, (name, i)
            at += up(size, unit)
        assert p[("files_bytes", "coef_bytes", "plane_bytes", "out_bytes")[k]] == at
    assert (d["entropy_begin"] + d["entropy_bytes"] == d["file_bytes"]).all()
    t = p["tables"][0]
    q = parsed[0]
    assert np.array_equal(t["quant"], q["quant"]) and np.array_equal(t["ac"][1]["counts"], q["ac"][1][0]) and np.array_equal(t["dc"][0]["values"], q["dc"][0][1])
    assert not t["dc"][2]["counts"].any() and not t["ac"][3]["values"].any()
    with pytest.raises(ValueError, match="2 GiB"):
        jpeg.plan([dict(parsed[0], nbytes=1 << 31)])


# ---- the range rule ----------------------------------------------------------------------------------------------------------------------
def test_the_pass_forms_stay_below_two_to_the_31():
    """Every intermediate and output of one 1-D pass is a linear form of the eight inputs; the largest absolute coefficient sum bounds the
    magnitude for inputs in int16."""
    from egogaussian_amd import jpeg
    forms = jpeg.idct_forms()
    worst = int(np.abs(forms).sum(axis=1).max())
    assert worst == jpeg.PASS_ABS_SUM and worst < 65536
    assert 32768 * worst + (1 << 17) < 1 << 31


def test_worst_sign_blocks_at_the_bounds_agree_in_int32_and_python_ints():
    from egogaussian_amd import jpeg
    forms = jpeg.idct_forms()
    outputs = forms[-8:]                                                 # the eight outputs before the descale
    rows = []
    for f in list(outputs) + list(forms[np.argsort(np.abs(forms).sum(axis=1))[-4:]]):
        for lo, hi in ((-32768, 32767), (-32767, 32768 - 1)):
            rows.append([hi if c > 0 else lo for c in f])
            rows.append([lo if c > 0 else hi for c in f])
    rows = np.array(rows, dtype=np.int64)
    for shift in (11, 18):
        exact = np.array([jpeg.idct_pass([int(v) for v in r], shift) for r in rows])              # Python ints
        with np.errstate(over="raise"):
            narrow = np.stack(jpeg.idct_pass([rows[:, k].astype(np.int32) for k in range(8)], shift), axis=1)
        assert narrow.dtype == np.int32 and np.array_equal(narrow, exact), shift
        log = []
        for r in rows:
            jpeg.idct_pass([int(v) for v in r], shift, log)
        assert max(abs(v) for v in log) < 1 << 31
    # whole blocks: a first row of +-8191 makes every workspace value +-32 764, with the worst signs of each output among the patterns
    rng = np.random.default_rng(5)
    signs = np.concatenate([np.sign(outputs), -np.sign(outputs), np.where(rng.random((48, 8)) < 0.5, -1, 1)]).astype(np.int64)
    blocks = np.zeros((len(signs), 8, 8), dtype=np.int16)
    blocks[:, 0, :] = 8191 * signs
    wide = jpeg.idct_blocks(blocks.reshape(-1, 64), dtype=np.int64)
    assert np.array_equal(wide, jpeg.idct_blocks(blocks.reshape(-1, 64), dtype=np.int32)) and wide.min() == 0 and wide.max() == 255


def test_one_step_outside_the_bounds_is_refused():
    from egogaussian_amd import jpeg
    ok = np.zeros((1, 64), dtype=np.int16)
    ok[0, 0] = 8191                                                     # 4 x 8191 = 32 764: the largest DC whose workspace is in range
    assert jpeg.idct_blocks(ok)[0, 0, 0] == 255
    ok[0, 0] = 8192
    with pytest.raises(jpeg.StatusError) as e:
        jpeg.idct_blocks(ok)
    assert e.value.status == 9
    ok[0, 0] = -8192                                                    # -32 768 exactly: inside
    assert jpeg.idct_blocks(ok)[0, 0, 0] == 0
    ok[0, 0] = -8193
    with pytest.raises(jpeg.StatusError):
        jpeg.idct_blocks(ok)
    W, H = 16, 16
    for dc, q, status in ((128, 255, 9), (128, 128, None), (257, 128, 8), (-256, 128, 9), (-257, 128, 8), (64, 128, None)):
        b = np.zeros((6, 64), dtype=np.int64)
        b[:, 0] = dc
        data = JC.write(b, W, H, quant=q)
        if status is None:
            if abs(dc * q) * 4 <= 32767:
                assert jpeg.decode(data).shape == (H, W, 3)
            else:
                with pytest.raises(jpeg.StatusError) as e:
                    jpeg.decode(data)
                assert e.value.status == 9
        else:
            with pytest.raises(jpeg.StatusError) as e:
                jpeg.decode(data)
            assert e.value.status == status, (dc, q)


# ---- the test writer and the malformed files ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(JC.written()))
def test_the_writers_files_round_trip(name):
    from egogaussian_amd import jpeg
    data, coef, (W, H, C, hs, vs) = JC.written()[name]
    p = jpeg.parse(data)
    assert (p["W"], p["H"], p["C"], p["hs"], p["vs"]) == (W, H, C, hs, vs)
    assert np.array_equal(jpeg.entropy_decode(data, p), coef)
    assert jpeg.decode(data).shape == (H, W, C)


@pytest.mark.parametrize("name", list(JC.malformed()))
def test_malformed_files_pass_parse_and_give_their_status(name):
    from egogaussian_amd import jpeg
    data, status = JC.malformed()[name]
    jpeg.parse(data)
    with pytest.raises(jpeg.StatusError) as e:
        jpeg.decode(data)
    assert e.value.status == status and jpeg.status_text(status) in str(e.value)
    assert set(jpeg.STATUS) == set(range(1, 10))


def test_the_reader_has_no_cpu_path():
    from egogaussian_amd import jpeg
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.JpegReader("cpu")
