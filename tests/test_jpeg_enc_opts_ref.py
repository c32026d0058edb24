"""tests/jpeg_enc_opts_ref.py, the rule of the JPEG encoder's options (restart intervals, optimised Huffman
tables) in numpy, against libjpeg: the files Pillow wrote (tests/golden/jpeg_encode_opts_cases.npz, no Pillow needed), a
random matrix against the Pillow on the machine, and jpeg_enc_ref.encode where every option is off."""
import io
import os
import re

import numpy as np
import pytest

import jpeg_enc_opts_ref
import jpeg_enc_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_opts_cases.npz")


def golden_cases():
    """name -> (frame, quality, sampling, restart_rows, restart_blocks, optimize, file bytes)"""
    z = np.load(GOLD)
    out = {}
    for n in z["names"].tolist():
        frame = z["frame/" + n] if "frame/" + n in z.files else getattr(jpeg_enc_opts_ref, str(z["formula/" + n]))()
        q, rr, rb, opt = (int(v) for v in z["options/" + n])
        out[n] = (frame, q, str(z["sampling/" + n]), rr, rb, bool(opt), z["file/" + n].tobytes())
    return out


def test_the_rule_writes_every_golden_file():
    cases = golden_cases()
    assert len(cases) == 30
    info = {}
    for name, (frame, q, s, rr, rb, opt, want) in cases.items():
        info[name] = {}
        assert jpeg_enc_opts_ref.encode(frame, q, s, rr, rb, opt, info[name]) == want, name
    scan = lambda n: cases[n][-1][info[n]["header"]:-2]
    # what the cases are there for: a numbering that wraps four times, rows that win, DRI without a marker, a stuffed pad byte
    # in front of a marker, the clamp, one-symbol tables, and a code that the limiting to 16 bits has to shorten
    assert info["37x53_444_r0_b1"]["segments"] == 35 and len(re.findall(b"\xff[\xd0-\xd7]", scan("37x53_444_r0_b1"))) >= 34
    assert info["37x53_420_r1_b5"]["interval"] == 4 and cases["37x53_420_r1_b5"][-1] == cases["37x53_420_r1_b0"][-1]
    for name in ("1x1_b1", "8x8_b1", "8x8_grey_r1"):
        assert info[name]["segments"] == 1 and b"\xff\xdd\x00\x04\x00\x01" in cases[name][-1] and not re.search(b"\xff[\xd0-\xd7]", scan(name))
    assert re.search(b"\xff\x00\xff[\xd0-\xd7]", scan("100x200_noise_q95_b7"))
    assert info["clamp_r32"]["interval"] == 65535 and info["clamp_r32"]["segments"] == 2
    assert b"\xff\xdd\x00\x04\xff\xff\xff\xda" in cases["clamp_r32"][-1] and scan("clamp_r32").count(b"\xff\xd0") == 1
    assert info["fibonacci_opt"]["max_unlimited"] >= 17 and len(cases["fibonacci_opt"][-1]) == 7774
    flat = cases["flat128_opt"][-1]
    assert [flat[m.start() + 3] for m in re.finditer(b"\xff\xc4", flat)] == [20] * 4        # 2 + 1 + 16 + one symbol
    for name, (frame, q, s, rr, rb, opt, want) in cases.items():
        if opt:
            assert info[name]["header"] <= len(jpeg_enc_ref.header(*frame.shape, q, s)) + 6, name


def test_with_every_option_off_it_is_the_default_rule():
    rng = np.random.default_rng(11)
    for shape, q, s in (((37, 53, 3), 75, "420"), ((9, 17, 3), 30, "444"), ((17, 33, 3), 90, "422"), ((20, 11, 1), 60, "420")):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        assert jpeg_enc_opts_ref.encode(a, q, s) == jpeg_enc_ref.encode(a, q, s)
        assert jpeg_enc_opts_ref.encode(a, q, s, 0, 0, False) == jpeg_enc_ref.encode(a, q, s)
    assert jpeg_enc_opts_ref.encode(a[..., 0], 60) == jpeg_enc_ref.encode(a, 60)


def test_the_optimal_table_of_a_few_counts():
    # one symbol: it and the reserved point get one bit each, the reserved point leaves
    assert jpeg_enc_opts_ref.gen_optimal_table([0] * 5 + [9] + [0] * 250) == ((1,) + (0,) * 15, (5,))
    # equal counts: ties go to the larger symbol, so the smaller symbols keep the shorter codes
    counts = [0] * 256
    counts[3] = counts[4] = counts[7] = 1
    bits, vals = jpeg_enc_opts_ref.gen_optimal_table(counts)
    assert (bits[:3], vals) == ((0, 3, 0), (3, 4, 7))       # with the reserved point: four codes of two bits, one leaves
    # counts 1, 2, 4 ... 2^19 behind the reserved 1: every merge adds a leaf to one chain, 20 bits unlimited, 16 after the
    # limiting, still a prefix code (Kraft)
    info = {}
    bits, vals = jpeg_enc_opts_ref.gen_optimal_table([1 << i for i in range(20)] + [0] * 236, info)
    assert info["max_unlimited"] == 20 and sum(bits) == 20 and vals[0] == 19 and bits[15] > 0
    assert sum(b * 2 ** (16 - l) for l, b in enumerate(bits, 1)) < 2 ** 16


def test_random_matrix_against_pillow():
    """240 cases over grey and RGB, the three samplings, q 1 .. 100, restart_marker_rows 0 .. 3, restart_marker_blocks 0 .. 11 and
    optimize on and off: whole files."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(20261019)
    bad, seen = [], set()
    for i in range(240):
        C, s = (1, "420") if rng.integers(0, 4) == 0 else (3, ("444", "422", "420")[int(rng.integers(0, 3))])
        H, W = (int(v) for v in rng.integers(1, 49, 2))
        a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        if i % 5 == 0:
            a = (a // 86 * 100).astype(np.uint8)             # few levels: short tables, long runs
        elif i % 5 == 1:
            a = np.broadcast_to((np.arange(W) * 5 + i).astype(np.uint8)[None, :, None], (H, W, C)).copy()
        q = int(rng.integers(1, 101))
        rr, rb, opt = (int(rng.integers(0, 4)) * int(rng.integers(0, 2)), int(rng.integers(0, 12)) * int(rng.integers(0, 2)),
                       bool(rng.integers(0, 2)))
        seen.add((C, s, rr > 0, rb > 0, opt))
        bio = io.BytesIO()
        kw = dict(format="JPEG", quality=q, restart_marker_rows=rr, restart_marker_blocks=rb, optimize=opt)
        if C == 3:
            kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[s]
        Image.fromarray(a[..., 0] if C == 1 else a).save(bio, **kw)
        if jpeg_enc_opts_ref.encode(a, q, s, rr, rb, opt) != bio.getvalue():
            bad.append((H, W, C, q, s, rr, rb, opt))
    assert not bad, bad
    assert len(seen) >= 24
