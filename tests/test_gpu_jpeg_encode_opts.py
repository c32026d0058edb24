"""The options of the device JPEG encoder (vf_jpeg_encode_opts, DESIGN.md 5.8: restart intervals, optimised Huffman tables)
against libjpeg: every file equals, byte for byte, the file Pillow wrote (tests/golden/jpeg_encode_opts_cases.npz) or the
numpy restatement of the rule (tests/jpeg_enc_opts_ref.py, itself held to Pillow by tests/test_jpeg_enc_opts_ref.py); alone
and in a batch, from bytes and from floats; the device decoder reads the files back; and the Python entry points pass the
options through.  No Pillow needed."""
import os
import re

import numpy as np
import pytest
import torch

import jpeg_enc_opts_ref
import jpeg_enc_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_opts_cases.npz")
_gold = {}


def gold():
    """name -> (frame, quality, sampling, restart_rows, restart_blocks, optimize, file bytes), and the archive; read once"""
    if not _gold:
        z = np.load(GOLD)
        _gold["z"] = z
        _gold["cases"] = {}
        for n in z["names"].tolist():
            frame = z["frame/" + n] if "frame/" + n in z.files else getattr(jpeg_enc_opts_ref, str(z["formula/" + n]))()
            q, rr, rb, opt = (int(v) for v in z["options/" + n])
            _gold["cases"][n] = (frame, q, str(z["sampling/" + n]), rr, rb, bool(opt), z["file/" + n].tobytes())
    return _gold["cases"], _gold["z"]


def enc(frames, quality=75, subsampling="420", restart_rows=0, restart_blocks=0, optimize=False):
    from video_filler_amd.data import encode_jpeg
    return encode_jpeg(frames, quality, subsampling, restart_rows=restart_rows, restart_blocks=restart_blocks, optimize=optimize)


def first_difference(got, want):
    n = min(len(got), len(want))
    d = np.flatnonzero(np.frombuffer(got[:n], np.uint8) != np.frombuffer(want[:n], np.uint8))
    return "%d bytes against %d, first difference at %s" % (len(got), len(want), int(d[0]) if d.size else "the end of the shorter")


def check(names):
    cases, _ = gold()
    bad = []
    for name in names:
        frame, q, s, rr, rb, opt, want = cases[name]
        (got,) = enc(frame[None], q, s, rr, rb, opt)
        if got != want:
            bad.append("%s: %s" % (name, first_difference(got, want)))
    assert not bad, "\n".join(bad)


def test_restart_intervals_at_every_sampling(hipb):
    """37 x 53: dummies to the right and below at a segment's start; 34 markers at 4:4:4 with an interval of 1, so the numbering
    wraps four times; rows win over blocks; 1 x 1 and 8 x 8: DRI and no marker"""
    cases, _ = gold()
    names = [n for n in cases if re.match(r"37x53_.*_r\d_b\d$", n)] + ["1x1_b1", "8x8_b1", "8x8_grey_r1"]
    assert len(names) == 20
    assert len(re.findall(b"\xff[\xd0-\xd7]", cases["37x53_444_r0_b1"][-1])) >= 34 and cases["37x53_420_r1_b5"][-1] == cases["37x53_420_r1_b0"][-1]
    check(names)


def test_segments_across_tiles_and_chunks_and_a_stuffed_pad_byte(hipb):
    """100 x 200 noise at quality 95, 4:4:4, an interval of 7: segments of 21 blocks straddle the tiles of 256 blocks, the
    stream covers several chunks of 4096 bytes, and a pad byte that comes out 0xFF is stuffed in front of its marker"""
    cases, _ = gold()
    want = cases["100x200_noise_q95_b7"][-1]
    assert re.search(b"\xff\x00\xff[\xd0-\xd7]", want) and len(want) > 12 * 4096
    check(["100x200_noise_q95_b7"])


def test_the_interval_is_clamped_to_what_dri_can_say(hipb):
    """264 x 16384 grey, restart_rows=32: 65536 MCUs asked for, DRI 0xFFFF and one RST0 written"""
    cases, _ = gold()
    want = cases["clamp_r32"][-1]
    assert b"\xff\xdd\x00\x04\xff\xff\xff\xda" in want
    check(["clamp_r32"])


def test_optimised_tables(hipb):
    """flat frames: one-symbol tables; RGB noise at 4:2:0: Cb and Cr share tables; with an interval: the predictor resets are
    in the counts; the Fibonacci frame: the unlimited code is longer than 16 bits and is cut down"""
    cases, _ = gold()
    names = [n for n in cases if n.endswith("_opt")]
    assert len(names) == 8
    check(names)


def test_a_batch_with_both_options_holds_the_files_of_its_frames(hipb):
    """five different frames in one call: the headers differ in length, the files stand at `offsets`, n = 1 gives the same
    files, and so do a device tensor and a float tensor through the byte rule"""
    cases, _ = gold()
    base = cases["37x53_444_r0_b1"][0]
    frames = np.stack([base, base[::-1].copy(), (base // 64 * 64).astype(np.uint8), 255 - base, np.full_like(base, 99)])
    for q, s, rr, rb, opt in ((75, "420", 0, 3, True), (90, "422", 1, 0, True), (60, "444", 0, 2, False), (100, "444", 2, 1, True)):
        info = [{} for _ in frames]
        want = [jpeg_enc_opts_ref.encode(f, q, s, rr, rb, opt, i) for f, i in zip(frames, info)]
        if opt:
            assert len({i["header"] for i in info}) >= 2
        files = enc(frames, q, s, rr, rb, opt)
        assert files == want, [first_difference(a, b) for a, b in zip(files, want) if a != b]
        assert [enc(f[None], q, s, rr, rb, opt)[0] for f in frames] == want             # n = 1
        assert enc(torch.from_numpy(frames).cuda(), q, s, rr, rb, opt) == want          # a device tensor
    buf, offsets = hipb.jpeg_encode(torch.from_numpy(frames).cuda(), 75, "420", restart_blocks=3, optimize=True)
    offs = offsets.cpu().tolist()
    want = [jpeg_enc_opts_ref.encode(f, 75, "420", 0, 3, True) for f in frames]
    assert offs == [0] + np.cumsum([len(w) for w in want]).tolist() and offs[-1] <= buf.numel()
    assert buf[:offs[-1]].cpu().numpy().tobytes() == b"".join(want)
    grey = np.ascontiguousarray(frames[..., 1:2])
    assert enc(grey, 60, "444", 1, 0, True) == [jpeg_enc_opts_ref.encode(f, 60, "420", 1, 0, True) for f in grey]
    # floats: image.savePNG's rule on the host, then the same files
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.25, 1.25, (5, 3, 37, 53)).astype(np.float32)
    v = np.minimum(np.maximum(x, np.float32(0)), np.float32(1))
    b = (np.float32(255) * v).astype(np.uint8).transpose(0, 2, 3, 1).copy()
    want = [jpeg_enc_opts_ref.encode(f, 80, "420", 1, 0, True) for f in b]
    assert enc(torch.from_numpy(x), 80, "420", 1, 0, True) == want
    assert enc(torch.from_numpy(x).cuda(), 80, "420", 1, 0, True) == want


def test_every_option_off_is_the_default_file(hipb):
    """the defaults go through vf_jpeg_encode; vf_jpeg_encode_opts with 0, 0, 0 writes the same bytes within the same bounds"""
    from video_filler_amd import backend
    cases, _ = gold()
    frame = cases["37x53_444_r0_b1"][0]
    want = jpeg_enc_ref.encode(frame, 75, "420")
    assert enc(frame[None]) == [want]
    t = torch.from_numpy(frame[None].copy()).cuda()
    pair = backend.jpeg_encode_opts_workspace_bytes(1, 37, 53, 3, "420")
    assert pair == backend.jpeg_encode_workspace_bytes(1, 37, 53, 3, "420")
    buf, offsets = hipb._encode("vf_jpeg_encode_opts", "jpeg_enc", t, 1, pair, 1, 1, 37, 53, 3, 75, 2, 0, 0, 0)
    offs = offsets.cpu().tolist()
    assert buf[:offs[1]].cpu().numpy().tobytes() == want


def test_round_trip_through_the_device_decoder(hipb):
    """data.decode_jpeg of the device's files is Pillow's decode of Pillow's (equal) files; data.jpeg_info finds the interval
    and the segments the options asked for"""
    from video_filler_amd import data
    cases, z = gold()
    names = [n for n in cases if "decoded/" + n in z.files]
    assert len(names) >= 25
    for name in names:
        frame, q, s, rr, rb, opt, want = cases[name]
        files = enc(frame[None], q, s, rr, rb, opt)
        assert files == [want], name
        (got,) = data.decode_jpeg(files)
        assert np.array_equal(got.cpu().numpy(), z["decoded/" + name]), name
        info = {}
        jpeg_enc_opts_ref.encode(frame, q, s, rr, rb, opt, info)
        found = data.jpeg_info(files[0])
        assert (found["restart_interval"], found["segments"]) == (info["interval"], info["segments"]), name
    assert data.jpeg_info(cases["37x53_444_r0_b1"][-1])["segments"] == 35


def test_save_frames_jpg_and_display_jpeg_pass_the_options_through(hipb, tmp_path):
    from video_filler_amd import inference
    rng = np.random.default_rng(3)
    groups = [torch.from_numpy(rng.uniform(-0.1, 1.1, (2, 3, 24, 40)).astype(np.float32)) for _ in range(3)]
    d = str(tmp_path / "frames")
    paths = inference.save_frames_jpg(d, *groups, quality=80, subsampling="422", restart_rows=1, optimize=True)
    want = enc(torch.cat(groups, 0), 80, "422", 1, 0, True)
    assert len(paths) == 6 and want != enc(torch.cat(groups, 0), 80, "422")
    for p, w in zip(paths, want):
        with open(p, "rb") as fh:
            got = fh.read()
        assert got == w and b"\xff\xdd\x00\x04\x00\x03" in got
    pack = torch.from_numpy(rng.uniform(-1, 1, (6, 3, 16, 16)).astype(np.float32))
    sheet = inference.display_tensor(pack, nrow=3, padding=2)
    jpg = inference.display_jpeg(pack, quality=85, restart_blocks=2, optimize=True, nrow=3, padding=2)
    assert jpg == enc(sheet.unsqueeze(0), 85, "420", 0, 2, True)[0]
    assert b"\xff\xdd\x00\x04\x00\x02" in jpg and len(jpg) < len(inference.display_jpeg(pack, quality=85, restart_blocks=2, nrow=3, padding=2))


def test_refusals_name_the_option(hipb):
    from video_filler_amd._lib import VfError
    t = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="restart_blocks = 65536"):
        hipb.jpeg_encode(t, 75, "420", restart_blocks=65536)
    with pytest.raises(ValueError, match="restart_rows=70000"):
        enc(np.zeros((1, 8, 8, 3), np.uint8), restart_rows=70000)
    pair = (1 << 20, 1 << 20)
    with pytest.raises(VfError, match="optimize = 2"):
        hipb._encode("vf_jpeg_encode_opts", "jpeg_enc", t, 1, pair, 1, 1, 8, 8, 3, 75, 2, 0, 0, 2)
