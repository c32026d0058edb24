"""tests/jpeg_enc_prog_ref.py, the rule of the progressive JPEG encoder (jpeg_simple_progression, jcphuff.c) in
numpy, against libjpeg: the files Pillow wrote (tests/golden/jpeg_encode_prog_cases.npz, no Pillow needed), what the cases
are there for as the rule's own counters report it, and a random sweep against the Pillow on the machine."""
import re

import numpy as np
import pytest

import jpeg_enc_prog_ref as P
import jpeg_prog_ref

_state = {}


def golden():
    """name -> (frame, quality, sampling, file), and the rule's info per name; read and encoded once"""
    if not _state:
        _state["cases"] = P.load_golden()
        _state["info"] = {}
        _state["bad"] = []
        for name, (frame, q, s, want) in _state["cases"].items():
            _state["info"][name] = {}
            if P.encode(frame, q, s, _state["info"][name]) != want:
                _state["bad"].append(name)
    return _state["cases"], _state["info"]


def per_scan(info, name, key):
    return [sc[key] for sc in info[name]["scans"]]


def test_the_rule_writes_every_golden_file():
    cases, _ = golden()
    assert len(cases) == 25 and not _state["bad"], _state["bad"]


def test_the_scan_script_and_the_segments_of_a_file():
    cases, _ = golden()
    for name, scans in (("37x53_420_q75", P.SCANS_COLOUR), ("8x8_grey", P.SCANS_GREY)):
        f = cases[name][3]
        assert f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9" and f.count(b"\xff\xc2") == 1 and b"\xff\xc0" not in f[:200]
        parsed = jpeg_prog_ref.parse(f)["scans"]
        assert [(tuple(sc["components"]), sc["Ss"], sc["Se"], sc["Ah"], sc["Al"]) for sc in parsed] == list(scans)
        # every scan but the DC refinement behind its own DHT; the colour DC scan behind two
        assert len(re.findall(b"\xff\xc4", f)) == len(scans) - 1 + (len(scans) == 10)
    # Cb and Cr have tables of their own: the two DHT 0x11 of the first chroma scans differ
    f = cases["37x53_444_q95"][3]
    ac1 = [m.start() for m in re.finditer(b"\xff\xc4..\x11", f, re.S)]
    assert len(ac1) == 4 and f[ac1[0]:ac1[0] + 40] != f[ac1[1]:ac1[1] + 40]


def test_what_the_cases_are_there_for():
    cases, info = golden()
    for name in ("1x1_grey", "1x1_444", "1x1_420", "8x8_grey", "8x8_422"):      # one block a scan: every run ends with the scan
        runs = per_scan(info, name, "eob_runs")
        assert max(runs) <= 1 and sum(per_scan(info, name, "cut_7fff")) == 0, name
    for name in ("flat16_grey", "flat16_rgb"):                                  # one-symbol tables, a single run per AC scan
        dc = [i for i, sc in enumerate(P.scan_script(cases[name][0].shape[2])) if sc[2] == 0]
        assert [r for i, r in enumerate(per_scan(info, name, "eob_runs")) if i not in dc] == [1] * (len(info[name]["scans"]) - 2)
        assert all(int((c > 0).sum()) == 1 for i, sc in enumerate(info[name]["scans"]) if i not in dc for c in sc["counts"].values())
    assert per_scan(info, "flat_grey_long", "cut_7fff") == [0, 1, 1, 1, 0, 1]
    assert per_scan(info, "flat_grey_long", "eob_runs") == [0, 2, 2, 2, 0, 2] and len(cases["flat_grey_long"][3]) < 14000
    # 64 x 64 noise at quality 100 does not reach the 937-bit limit (every block brings a symbol); the frame built for it does,
    # in both refinement scans, and has refinement ZRLs
    assert sum(per_scan(info, "noise_q100_444", "flush_937")) == 0
    flush = per_scan(info, "flush_grey_q100", "flush_937")
    assert flush[3] >= 1 and flush[5] >= 1 and sum(flush) == flush[3] + flush[5]
    assert sum(per_scan(info, "flush_grey_q100", "zrl_refine")) >= 1
    f = cases["100x200_noise_q95_444"][3]
    assert b"\xff\x00" in f and len(f) > 8 * 4096 and 13 * 25 > 256
    busy = per_scan(info, "busy_left_grey", "eob_runs")
    assert min(busy[1:4] + busy[5:]) >= 2                       # runs of 504 flat blocks, ended by the next row's busy blocks
    z = per_scan(info, "zrl_444_q90", "zrl_first")
    assert z[4] >= 1 and z[2] >= 1 and z[3] >= 1, z              # Y 6 - 63, Cr, Cb
    assert info["fibonacci_grey_q50"]["max_unlimited"] >= 17


def test_a_dummy_carries_the_dc_of_the_previous_real_block():
    """37 x 53 at 4:2:0: 3 x 4 MCUs of 2 x 2 luma blocks over 5 x 7 real ones; the AC scans walk 35 luma blocks"""
    cases, info = golden()
    frame, q, s, want = cases["37x53_420_q75"]
    scans = info["37x53_420_q75"]["scans"]
    assert sum(int(c.sum()) for c in scans[0]["counts"].values()) == 3 * 4 * 6          # the DC scan: every block, dummies too
    coef, bw, bh = jpeg_prog_ref.coefficients(want)
    assert (bh[0], bw[0]) == (5, 7) and coef[0].shape[:2] == (6, 8)
    assert np.array_equal(coef[0][:5, 7, 0], coef[0][:5, 6, 0])                         # to the right: the block beside it


def test_random_sweep_against_pillow():
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(20261020)
    bad, seen = [], set()
    for i in range(120):
        C, s = (1, "420") if rng.integers(0, 4) == 0 else (3, ("444", "422", "420")[int(rng.integers(0, 3))])
        H, W = (int(v) for v in rng.integers(1, 49, 2))
        a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        if i % 5 == 0:
            a = (a // 86 * 100).astype(np.uint8)             # few levels
        elif i % 5 == 1:
            a = np.broadcast_to((np.arange(W) * 5 + i).astype(np.uint8)[None, :, None], (H, W, C)).copy()
        elif i % 5 == 2:
            a = (128 + (a.astype(np.int64) - 128) // 16).astype(np.uint8)      # faint: long EOB runs, refinement ZRLs
        q = int(rng.integers(1, 101))
        seen.add((C, s))
        if P.encode(a, q, s) != P.pillow_file(a, q, s):
            bad.append((H, W, C, q, s, i))
    assert not bad, bad
    assert len(seen) == 4
    a = rng.integers(0, 256, (24, 24, 3), dtype=np.uint8)
    assert P.pillow_file(a, 80, "420", optimize=True) == P.pillow_file(a, 80, "420")     # libjpeg forces optimize_coding


def test_golden_files_are_what_pillow_writes_today():
    pytest.importorskip("PIL.Image")
    cases, _ = golden()
    for name, (frame, q, s, want) in cases.items():
        assert P.pillow_file(frame, q, s) == want, name
