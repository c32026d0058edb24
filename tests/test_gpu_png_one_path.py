"""The default PNG entry is the full rule's pipeline in its one-pass, 8-bit, uint8 case (vf_png_decode.hip):
vf_png_decode and vf_png_decode_full (out_kind 0) give equal bytes and equal status words on every file the default rule
takes, alone and in one mixed batch, and each entry reports its own profiling labels.

The files: every good and corrupt fixture of tests/golden/png_decode_cases.npz, and five written here at the smallest shapes
at which the one-pass case can go wrong.  An image whose status is not 0 has no defined bytes; its status is compared."""
import os

import numpy as np
import pytest
import torch

import png_full_cases as cases
import png_load_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "png_decode_cases.npz"))


def _written():
    rgb = cases.random_pixels(70, 5, 2, 8, 21)
    few = cases.palette(2)[:3]
    ix = cases.random_pixels(6, 9, 3, 2, 22) % 3
    ix[4, 7] = 3                                           # the palette has three entries
    return {
        # two 64-row bands, and the unfiltered rows are the output
        "made/rgb_paeth_70x5": (cases.write_png(rgb, 2, 8, False, filters=4), 0),
        # sub-byte samples, two bytes per row with three bits of padding, expansion through the unfiltered rows
        "made/p1_trns_3x13": (cases.write_png(cases.random_pixels(3, 13, 3, 1, 23), 3, 1, False, seed=1, plte=cases.palette(1),
                                              trns=bytes([7, 200])), 0),
        # two bands; with channels=3 the rows are expanded, with the file's channels they are the output
        "made/la_66x3": (cases.write_png(cases.random_pixels(66, 3, 4, 8, 24), 4, 8, False, seed=2), 0),
        # the second band's wave finds the filter byte
        "made/rgb_filter7_row65": (cases.write_png(rgb, 2, 8, False, filters=4, force_filter={(0, 65): 7}), cases.STATUS["bad filter"]),
        "made/p2_index_3_of_3": (cases.write_png(ix, 3, 2, False, seed=3, plte=few), cases.STATUS["bad palette index"]),
    }


FILES = {"good/" + k[5:]: (GOLDEN[k].tobytes(), 0) for k in GOLDEN.files if k.startswith("good/")}
FILES.update({"bad/" + k[4:]: (GOLDEN[k].tobytes(), int(GOLDEN["status/" + k[4:]])) for k in GOLDEN.files if k.startswith("bad/")})
FILES.update(_written())


def _allowed(f, channels):
    """whether the byte rule has an output of `channels` for the file (png_out_channels of the library, restated)"""
    d = png_load_ref.parse(f)
    if channels is None:
        return not (d["trns"] is not None and d["color_type"] in (0, 2))
    return not (channels == 1 and d["color_type"] in (2, 3, 6))


def _images(res, n):
    """(out, offsets, status) of one call -> the n images' bytes (None where the status is not 0), the status words"""
    out, offs, status = res
    status = status.cpu().tolist()
    out = out.cpu().numpy()
    assert out.dtype == np.uint8 and len(status) == n
    return [out[offs[i]:offs[i + 1]].copy() if status[i] == 0 else None for i in range(n)], status


def _equal(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


def test_the_set_holds_what_it_should():
    assert sum(n.startswith("good/") for n in FILES) > 30 and sum(n.startswith("bad/") for n in FILES) >= 5
    made = {n: png_load_ref.parse(f) for n, (f, st) in FILES.items() if n.startswith("made/")}
    assert len(made) == 5 and all(d["supported"] for d in made.values())
    assert {st for f, st in FILES.values()} >= {0, 5, 7}


@pytest.mark.parametrize("channels", [None, 1, 3])
def test_both_entries_give_the_same_bytes_and_status_words(hipb, channels):
    names = [n for n in sorted(FILES) if _allowed(FILES[n][0], channels)]
    assert len(names) > 25 and sum(n.startswith("made/") for n in names) == (1 if channels == 1 else 5)   # grey+alpha alone has a grey
    alone = {}
    for n in names:
        f, want_status = FILES[n]
        (a,), sa = _images(hipb.png_decode([f], channels), 1)
        (b,), sb = _images(hipb.png_decode_full([f], channels, out_kind=0), 1)
        assert sa == sb == [want_status], n
        assert _equal(a, b), n
        if n.startswith("made/") and want_status == 0:
            assert np.array_equal(a, png_load_ref.load(f, channels).reshape(-1)), n
        alone[n] = a
    files = [FILES[n][0] for n in names]
    da, sa = _images(hipb.png_decode(files, channels), len(names))
    db, sb = _images(hipb.png_decode_full(files, channels, out_kind=0), len(names))
    assert sa == sb == [FILES[n][1] for n in names]
    for n, a, b in zip(names, da, db):
        assert _equal(a, alone[n]) and _equal(b, alone[n]), n


def test_each_entry_reports_its_own_labels(hipb):
    files = [FILES[n][0] for n in ("made/rgb_paeth_70x5", "made/p1_trns_3x13", "made/la_66x3")]
    hipb.png_decode(files)                                 # warm: workspace and staging are there
    hipb.png_decode_full(files)
    torch.cuda.synchronize()
    hipb.prof_begin()
    hipb.png_decode(files)
    st = hipb.prof_end()
    assert {k for k in st if k.startswith("pngd_")} == {"pngd_inflate", "pngd_unfilter", "pngd_expand"}, sorted(st)
    assert all(st[k]["launches"] == 1 for k in ("pngd_inflate", "pngd_unfilter", "pngd_expand"))
    hipb.prof_begin()
    hipb.png_decode_full(files)
    st = hipb.prof_end()
    assert {k for k in st if k.startswith("pngd_")} == {"pngd_inflate", "pngd_unfilter_full", "pngd_expand_full"}, sorted(st)
    assert all(st[k]["launches"] == 1 for k in ("pngd_inflate", "pngd_unfilter_full", "pngd_expand_full"))
