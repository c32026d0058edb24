"""The GIF decoder's definition (tests/gif_decode_ref.py) against its witnesses, on the host: Pillow on the
Pillow-agreed class of tests/gif_decode_cases.py, gif_ref.read_gif on the files the project's own encoder rule writes, and the
status, malformed and unsupported fixtures.  Every comparison is exact."""
import numpy as np
import pytest

import gif_cases
import gif_decode_cases as cases
import gif_decode_ref as R
import gif_ref


def test_the_fixture_set_is_the_one_the_tests_count_on():
    fx = cases.fixtures()
    kinds = {k: len(cases.of_kind(k)) for k in ("good", "corrupt", "malformed", "unsupported")}
    assert kinds == {"good": 37, "corrupt": 7, "malformed": 7, "unsupported": 1}, kinds
    assert len(fx) == sum(kinds.values())
    assert sum(n.startswith("pil/") for n in fx) == 10
    sizes = set()
    for n in cases.of_kind("good"):
        sizes |= {f["min_code_size"] for f in cases.reference(n)[2]["frame_info"]}
    assert sizes == set(range(2, 9))
    # Pillow writes minimum code size 8 whatever the palette; its 2, 4, 16 and 256 colours show in the table sizes
    assert [cases.reference("pil/p%d" % c)[2]["global_table_size"] for c in (2, 4, 16, 256)] == [4, 4, 16, 256]
    assert {f["min_code_size"] for c in (2, 4, 16, 256) for f in cases.reference("pil/p%d" % c)[2]["frame_info"]} == {8}
    assert cases.reference("hand/frames_70")[2]["frames"] == 70 and cases.reference("hand/screen_1x1")[2]["frames"] == 1
    # interlace: every pass is empty for one height and non-empty for another
    heights = {f["h"] for f in cases.reference("hand/interlaced")[2]["frame_info"] if f["interlace"]}
    assert heights == {1, 2, 3, 4, 5, 8, 9, 17}
    for start, step in ((4, 8), (2, 4), (1, 2)):
        assert any(len(range(start, h, step)) == 0 for h in heights) and any(len(range(start, h, step)) > 0 for h in heights)
    assert all(sorted(R.lace_order(h)) == list(range(h)) for h in range(1, 40))


def test_the_reference_equals_pillow_on_the_agreed_class():
    """Outside the class (a partial or transparent first frame, a disposal 2 that nothing repaints) Pillow fills with the
    background colour and the rule leaves the canvas transparent: there gif_decode_ref alone is the rule and nothing is
    compared."""
    labelled = [n for n in cases.of_kind("good") if cases.fixtures()[n].pillow]
    compared = 0
    for n in cases.of_kind("good"):
        c = cases.fixtures()[n]
        ref, status, _ = cases.reference(n)
        assert status == R.OK, n
        if not c.pillow:
            assert c.what, "%s is outside the Pillow-agreed class and says why" % n
            continue
        assert cases.agrees_with_pillow(c.data, ref), n
        compared += 1
    assert compared == len(labelled) == 30


def test_rgb_output_is_the_colour_planes_and_untouched_pixels_are_black():
    for n in ("hand/partial_first", "hand/d2_left_open", "hand/rects_d013"):
        rgba = cases.reference(n)[0]
        rgb, status, _ = R.decode(cases.fixtures()[n].data)
        assert status == 0 and np.array_equal(rgb, rgba[..., :3]) and set(np.unique(rgba[..., 3])) <= {0, 255}
        assert not rgba[..., :3][rgba[..., 3] == 0].any()
    assert (cases.reference("hand/partial_first")[0][0, ..., 3] == 0).sum() == 12 * 10 - 4 * 3
    # disposal 4 .. 7 is disposal 1
    data = cases.fixtures()["hand/rects_d4567"].data
    same = bytearray(data)
    at = [i for i in range(len(data) - 8) if data[i:i + 3] == b"\x21\xf9\x04" and data[i + 7] == 0]
    assert len(at) == 7
    for i in at:
        same[i + 3] = (same[i + 3] & 1) | 1 << 2
    assert np.array_equal(R.decode(bytes(same), True)[0], cases.reference("hand/rects_d4567")[0])


@pytest.mark.parametrize("geom", [(64, 64), (71, 59)])
def test_the_reference_reads_what_the_encoder_rule_writes(geom):
    """gif_ref.read_gif plus its table lookup, on every content kind at 64 x 64 and on one geometry above CHUNK"""
    H, W = geom
    frames = gif_cases.contents(H, W)
    assert "colours_256" in frames and ("boundary" in frames) == (H * W >= gif_ref.CHUNK)
    clip = np.stack(list(frames.values()))
    data = gif_ref.encode(clip, 7)
    strict = gif_ref.read_gif(data)
    want = np.stack([t[f] for t, f in zip(strict["tables"], strict["frames"])])
    got, status, meta = R.decode(data)
    assert status == 0 and np.array_equal(got, want)
    assert meta["loop"] == 0 and [f["delay"] for f in meta["frame_info"]] == strict["delays"] and meta["frames"] == len(clip)
    rgba = R.decode(data, alpha=True)[0]
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()


def test_writer_policies_round_trip_and_differ():
    idx = cases.noise_idx(64, 80, 256, 100)
    streams = {}
    for policy in ("standard", "deferred", "none"):
        codes = cases.lzw_codes(idx, 8, policy)
        streams[policy] = cases.pack_codes(codes, 8)
        got, status = R.unlzw(streams[policy], 8, idx.size)
        assert status == 0 and np.array_equal(got.reshape(idx.shape), idx), policy
        assert (codes[0] == 256) == (policy != "none")
    assert len(set(streams.values())) == 3
    assert cases.lzw_codes(idx, 8, "deferred").count(256) == 1 and len(cases.lzw_codes(idx, 8, "deferred")) > 4096
    # KwKwK: a constant run is the chain c, n, n + 1, ...
    codes = cases.lzw_codes(np.full(10, 3), 2)
    assert codes == [4, 3, 6, 7, 8, 5]
    # a stream that goes on behind the full rectangle, with no EOI, is read as far as the rectangle
    assert cases.reference("hand/extra_codes_behind_full")[1] == 0


def test_corrupt_malformed_and_unsupported_fixtures():
    seen = set()
    for n in cases.of_kind("corrupt"):
        c = cases.fixtures()[n]
        assert cases.reference(n)[1] == c.status != 0, n
        seen.add(c.status)
    assert seen == {R.BAD_CODE, R.SHORT_DATA, R.BAD_INDEX}
    for n in cases.of_kind("malformed"):
        with pytest.raises(R.GifMalformed):
            R.parse(cases.fixtures()[n].data)
    for n in cases.of_kind("unsupported"):
        meta = R.parse(cases.fixtures()[n].data)
        assert not meta["supported"] and cases.fixtures()[n].what in meta["reason"]
    # every truncation of a good file is malformed, never an exception of another kind
    data = cases.fixtures()["hand/extensions"].data
    end = data.index(b"\x3bjunk")
    for cut in range(end):
        with pytest.raises(R.GifMalformed):
            R.parse(data[:cut])
    assert R.parse(data[:end + 1])["frames"] == 2
