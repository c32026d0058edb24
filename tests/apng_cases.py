"""Fixtures of the animated-PNG decoder: files Pillow's writer makes (sub-rectangles, the three
disposals, default image in or out, per-frame durations), files assembled here chunk by chunk from frames that
png_full_cases.write_png encodes (every format the full PNG rule takes, Adam7, 16 bits, streams split into many fdATs),
and the malformed, unsupported and corrupt variants of them.  fixtures() builds them once."""
import io
import struct
import zlib

import numpy as np

import png_full_cases as pfc

SIG = b"\x89PNG\r\n\x1a\n"
_CACHE = {}


def chunk(typ, body=b""):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) & 0xFFFFFFFF)


def chunks_of(png):
    out, at = [], 8
    while at < len(png):
        (n,) = struct.unpack(">I", png[at:at + 4])
        out.append((png[at + 4:at + 8], png[at + 8:at + 8 + n]))
        at += 12 + n
    return out


def join(chunks):
    return SIG + b"".join(chunk(t, b) for t, b in chunks)


def fctl(seq, w, h, x=0, y=0, delay=(10, 100), dispose=0, blend=0):
    return struct.pack(">IIIIIHHBB", seq, w, h, x, y, delay[0], delay[1], dispose, blend)


def frame(pix, x=0, y=0, delay=(10, 100), dispose=0, blend=0, split=(), seed=0):
    return dict(pix=np.asarray(pix), x=x, y=y, delay=delay, dispose=dispose, blend=blend, split=split, seed=seed)


def chunk_list(W, H, ct, depth, frames, lace=False, plte=None, trns=None, plays=0, default=None, level=6):
    """The chunks [(type, body)] of an APNG: frames[0] in IDAT when default is None (it must cover the canvas), else `default`
    (samples H x W x rc) is the IDAT image and every frame is in fdATs.  Sequence numbers as the specification asks."""
    def parts(pix, split, seed):
        png = pfc.write_png(pix, ct, depth, lace, seed=seed, plte=plte, trns=trns, split=split, level=level)
        return [b for t, b in chunks_of(png) if t == b"IDAT"]
    out = [(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ct, 0, 0, int(lace)))]
    if plte is not None:
        out.append((b"PLTE", np.asarray(plte, np.uint8).tobytes()))
    if trns is not None:
        out.append((b"tRNS", bytes(trns)))
    out.append((b"acTL", struct.pack(">II", len(frames), plays)))
    seq = 0
    if default is not None:
        out += [(b"IDAT", p) for p in parts(default, (), 99)]
    for k, f in enumerate(frames):
        h, w = f["pix"].shape[:2]
        out.append((b"fcTL", fctl(seq, w, h, f["x"], f["y"], f["delay"], f["dispose"], f["blend"])))
        seq += 1
        for p in parts(f["pix"], f["split"], f["seed"] + k):
            if k == 0 and default is None:
                out.append((b"IDAT", p))
            else:
                out.append((b"fdAT", struct.pack(">I", seq) + p))
                seq += 1
    return out + [(b"IEND", b"")]


def build(*a, **kw):
    return join(chunk_list(*a, **kw))


def pix(H, W, ct, depth, seed):
    return pfc.random_pixels(H, W, ct, depth, seed)


def palette(depth, black0=True):
    """png_full_cases' palette; black0 puts black at entry 0: Pillow clears a palette file to INDEX 0 where the rule clears to
    transparent black, and the two agree in RGB only then (palette_dispose1_colour0 keeps a colour there, for the hand-computed test)"""
    p = pfc.palette(depth).copy()
    if black0:
        p[0] = 0
    return p


# ------------------------------------------------------------------------------------------------------- Pillow-written
def _pillow_frames(mode, n, H, W, seed):
    """frames that differ from one another inside a moving box, so that Pillow's writer crops sub-rectangles"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    c = {"L": 1, "RGB": 3, "RGBA": 4, "P": 1}[mode]
    base = rng.integers(0, 256 if mode != "P" else 16, (H, W, c), dtype=np.uint8)
    out = []
    for k in range(n):
        a = base.copy()
        y0, x0 = (3 * k) % (H - 4), (5 * k + 1) % (W - 6)
        a[y0:y0 + 4, x0:x0 + 6] = rng.integers(0, 256 if mode != "P" else 16, (4, 6, c), dtype=np.uint8)
        if mode == "RGBA":
            a[..., 3] = np.where(a[..., 3] > 128, 255, a[..., 3])
        if mode == "P":
            im = Image.frombytes("P", (W, H), a[..., 0].tobytes())
            im.putpalette(np.random.default_rng(7).integers(0, 256, 48, dtype=np.uint8).tobytes())
        else:
            im = Image.fromarray(a[..., 0] if c == 1 else a)
        out.append(im)
    return out


def pillow_written():
    out = {}
    for mode in ("RGB", "RGBA", "L", "P"):
        for disposal in (0, 1, 2):
            for default in (False, True):
                fr = _pillow_frames(mode, 4, 13, 17, len(out))
                b = io.BytesIO()
                try:
                    fr[0].save(b, format="PNG", save_all=True, append_images=fr[1:], duration=[30, 40, 50, 60], loop=2,
                               disposal=disposal, blend=0, default_image=default)
                except ValueError:                   # "images do not match": L and P with disposal 1 and 2 (hand-assembled below)
                    continue
                out["pillow_%s_d%d_%s" % (mode, disposal, "default" if default else "frame0")] = b.getvalue()
    return out


# ------------------------------------------------------------------------------------------------------- hand-assembled
def hand_assembled():
    g = {}
    W, H = 19, 14
    rgb = [pix(H, W, 2, 8, s) for s in range(4)]
    g["one_pixel_frame"] = build(W, H, 2, 8, [frame(rgb[0]), frame(pix(1, 1, 2, 8, 5), x=7, y=3), frame(pix(1, 1, 2, 8, 6), x=0, y=0)])
    g["edges"] = build(W, H, 2, 8, [frame(rgb[0]), frame(pix(5, 4, 2, 8, 7), x=W - 4, y=2, dispose=1),
                                    frame(pix(3, 6, 2, 8, 8), x=1, y=H - 3, dispose=2), frame(pix(2, 2, 2, 8, 9), x=W - 2, y=H - 2)])
    g["previous_first_frame0"] = build(W, H, 2, 8, [frame(rgb[0], dispose=2), frame(pix(4, 4, 2, 8, 10), x=2, y=2), frame(rgb[1])])
    g["previous_first_excluded_default"] = build(W, H, 2, 8, [frame(pix(6, 7, 2, 8, 11), x=3, y=4, dispose=2),
                                                            frame(pix(4, 4, 2, 8, 12), x=1, y=1)], default=rgb[2])
    g["background_then_smaller"] = build(W, H, 2, 8, [frame(rgb[0]), frame(pix(8, 9, 2, 8, 13), x=4, y=3, dispose=1),
                                                     frame(pix(3, 3, 2, 8, 14), x=6, y=5), frame(pix(2, 5, 2, 8, 15), x=0, y=0, dispose=1),
                                                     frame(pix(1, 1, 2, 8, 16), x=18, y=13)])
    g["over_without_alpha"] = build(W, H, 2, 8, [frame(rgb[0], blend=1), frame(pix(5, 5, 2, 8, 17), x=5, y=5, blend=1, dispose=2),
                                                 frame(pix(4, 9, 2, 8, 18), x=9, y=0, blend=1)])
    for d in (1, 2):
        g["grey_dispose%d" % d] = build(W, H, 0, 8, [frame(pix(H, W, 0, 8, 20)), frame(pix(6, 5, 0, 8, 21), x=2, y=3, dispose=d),
                                                     frame(pix(4, 7, 0, 8, 22), x=10, y=8, dispose=d), frame(pix(3, 3, 0, 8, 23), x=0, y=0)])
        pal = palette(4)
        g["palette_dispose%d" % d] = build(W, H, 3, 4, [frame(pix(H, W, 3, 4, 24)), frame(pix(6, 5, 3, 4, 25), x=2, y=3, dispose=d),
                                                        frame(pix(4, 7, 3, 4, 26), x=10, y=8, dispose=d), frame(pix(3, 3, 3, 4, 27))], plte=pal)
    g["palette_trns"] = build(W, H, 3, 8, [frame(pix(H, W, 3, 8, 28)), frame(pix(7, 7, 3, 8, 29), x=3, y=3, dispose=1),
                                           frame(pix(5, 9, 3, 8, 30), x=8, y=6, dispose=2), frame(pix(2, 2, 3, 8, 31), x=1, y=1)],
                              plte=palette(8), trns=bytes([0, 128, 255, 7, 9]))
    g["palette_dispose1_colour0"] = build(W, H, 3, 4, [frame(pix(H, W, 3, 4, 24)), frame(pix(6, 5, 3, 4, 25), x=2, y=3, dispose=1),
                                                       frame(pix(3, 3, 3, 4, 27))], plte=palette(4, black0=False))
    g["palette_1bit"] = build(W, H, 3, 1, [frame(pix(H, W, 3, 1, 32)), frame(pix(5, 11, 3, 1, 33), x=3, y=2)], plte=pfc.palette(1))
    g["grey_alpha"] = build(W, H, 4, 8, [frame(pix(H, W, 4, 8, 34)), frame(pix(6, 6, 4, 8, 35), x=4, y=4, dispose=1),
                                         frame(pix(5, 5, 4, 8, 36), x=9, y=2, dispose=2), frame(pix(3, 8, 4, 8, 37), x=0, y=11)])
    g["rgba"] = build(W, H, 6, 8, [frame(pix(H, W, 6, 8, 38), dispose=1), frame(pix(6, 6, 6, 8, 39), x=4, y=4),
                                   frame(pix(5, 5, 6, 8, 40), x=9, y=2, dispose=2), frame(pix(3, 8, 6, 8, 41), x=0, y=11)])
    g["adam7_rgb"] = build(W, H, 2, 8, [frame(rgb[0]), frame(pix(9, 10, 2, 8, 42), x=5, y=2, dispose=1), frame(pix(1, 1, 2, 8, 43), x=2, y=2),
                                        frame(pix(3, 2, 2, 8, 44), x=17, y=11)], lace=True)
    g["adam7_palette2"] = build(W, H, 3, 2, [frame(pix(H, W, 3, 2, 45)), frame(pix(9, 10, 3, 2, 46), x=5, y=2)], lace=True, plte=pfc.palette(2))
    g["rgb16"] = build(W, H, 2, 16, [frame(pix(H, W, 2, 16, 47)), frame(pix(6, 7, 2, 16, 48), x=3, y=3, dispose=2),
                                     frame(pix(4, 4, 2, 16, 49), x=15, y=10)])
    g["rgba16_adam7"] = build(W, H, 6, 16, [frame(pix(H, W, 6, 16, 50)), frame(pix(6, 7, 6, 16, 51), x=3, y=3, dispose=1),
                                            frame(pix(9, 9, 6, 16, 52), x=1, y=2)], lace=True)
    g["grey16"] = build(W, H, 0, 16, [frame(pix(H, W, 0, 16, 53)), frame(pix(6, 7, 0, 16, 54), x=3, y=3)])
    # stored blocks (level 0): one frame's stream in many fdATs, single-byte ones included, and frame 0's in several IDATs
    g["many_fdats"] = build(W, H, 2, 8, [frame(rgb[0], split=(1, 2, 3, 50, 51)), frame(pix(9, 11, 2, 8, 55), x=2, y=1,
                                                                                      split=(1, 2, 3, 7, 8, 9, 100, 101, 200, 299)),
                                         frame(rgb[3], split=tuple(range(1, 40)))], level=0)
    g["delay_den_0"] = build(W, H, 2, 8, [frame(rgb[0], delay=(7, 0)), frame(rgb[1], delay=(0, 0)), frame(rgb[2], delay=(65535, 65535))])
    g["excluded_default"] = build(W, H, 2, 8, [frame(rgb[1]), frame(pix(5, 5, 2, 8, 56), x=3, y=3, dispose=1), frame(pix(4, 4, 2, 8, 57), x=0, y=0)],
                                  default=rgb[0])
    g["one_frame"] = build(W, H, 2, 8, [frame(rgb[2])], plays=5)
    g["wide_127"] = build(127, 64, 0, 8, [frame(pix(64, 127, 0, 8, 58)), frame(pix(64, 127, 0, 8, 59)), frame(pix(33, 65, 0, 8, 60), x=62, y=31)])
    g["plain_png"] = pfc.write_png(rgb[0], 2, 8)
    g["plain_png_adam7_ga16"] = pfc.write_png(pix(9, 17, 4, 16, 61), 4, 16, True)
    plain = chunks_of(g["plain_png"])     # fcTL / fdAT without acTL are chunks nobody reads
    g["plain_png_stray_fctl"] = join(plain[:1] + [(b"fcTL", fctl(5, 3, 3)), (b"fdAT", b"\0\0\0\x09junk")] + plain[1:])
    return g


# ------------------------------------------------------------------------------------- malformed, unsupported, corrupt
def _base():
    W, H = 19, 14
    return W, H, chunk_list(W, H, 2, 8, [frame(pix(H, W, 2, 8, 70)), frame(pix(5, 6, 2, 8, 71), x=2, y=3, split=(9,)),
                                         frame(pix(4, 4, 2, 8, 72), x=10, y=9)])


def _set(ch, i, body):
    return ch[:i] + [(ch[i][0], body)] + ch[i + 1:]


def malformed():
    """name -> (file, a word of the reason)"""
    W, H, ch = _base()
    ty = [t for t, _ in ch]
    assert ty == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    good = join(ch)
    m = {}
    for name, i in (("crc_ihdr", 0), ("crc_actl", 1), ("crc_fctl", 4), ("crc_idat", 3), ("crc_fdat", 6), ("crc_iend", 9)):
        at = len(join(ch[:i + 1])) - 1
        m[name] = (good[:at] + bytes([good[at] ^ 1]) + good[at + 1:], "CRC")
    m["second_actl"] = (join(ch[:2] + [ch[1]] + ch[2:]), "second acTL")
    m["actl_after_idat"] = (join(ch[:1] + ch[2:4] + [ch[1]] + ch[4:]), "acTL after IDAT")
    m["actl_short"] = (join(_set(ch, 1, ch[1][1][:7])), "acTL of 7 bytes")
    m["fewer_fctl"] = (join(_set(ch, 1, struct.pack(">II", 4, 0))), "acTL says 4")
    m["more_fctl"] = (join(_set(ch, 1, struct.pack(">II", 2, 0))), "acTL says 2")
    m["zero_frames"] = (join(_set(ch, 1, struct.pack(">II", 0, 0))), "num_frames is 0")
    m["seq_missing"] = (join(_set(ch, 6, struct.pack(">I", 4) + ch[6][1][4:])), "sequence number 4, 3 is due")
    m["seq_repeated"] = (join(_set(ch, 5, struct.pack(">I", 1) + ch[5][1][4:])), "sequence number 1, 2 is due")
    m["seq_out_of_order"] = (join(ch[:5] + [ch[6], ch[5]] + ch[7:]), "is due")
    m["seq_fctl_wrong"] = (join(_set(ch, 7, struct.pack(">I", 7) + ch[7][1][4:])), "fcTL")
    m["seq_first_not_0"] = (join(_set(ch, 2, struct.pack(">I", 1) + ch[2][1][4:])), "0 is due")
    m["fdat_before_fctl"] = (join(ch[:2] + [(b"fdAT", struct.pack(">I", 0) + b"xx")] + ch[2:]), "before the first fcTL")
    m["fdat_short"] = (join(_set(ch, 6, b"\0\0\0")), "fdAT of 3 bytes")
    m["fdat_in_idat_frame"] = (join(ch[:4] + [(b"fdAT", struct.pack(">I", 1) + b"xx")] + ch[4:]), "IDAT chunks hold")
    m["frame_no_data"] = (join(ch[:8] + [ch[9]]), "frame 2 has no data")
    m["frame_empty_fdat"] = (join(ch[:8] + [(b"fdAT", struct.pack(">I", 5))] + [ch[9]]), "frame 2 has no data")
    m["two_fctl_no_data_between"] = (join(ch[:5] + [(b"fcTL", fctl(2, 4, 4, 10, 9)), (b"fdAT", struct.pack(">I", 3) + ch[8][1][4:]), ch[9]]),
                                     "frame 1 has no data")
    m["zero_width"] = (join(_set(ch, 4, fctl(1, 0, 5, 2, 3))), "frame 1 is 0x5")
    m["zero_height"] = (join(_set(ch, 4, fctl(1, 6, 0, 2, 3))), "frame 1 is 6x0")
    m["leaves_right"] = (join(_set(ch, 4, fctl(1, 6, 5, W - 5, 3))), "leaves the 19x14 canvas")
    m["leaves_bottom"] = (join(_set(ch, 4, fctl(1, 6, 5, 2, H - 4))), "leaves the 19x14 canvas")
    m["leaves_far"] = (join(_set(ch, 4, fctl(1, 6, 5, 0xFFFFFFFF, 0))), "leaves")
    m["first_not_canvas"] = (join(_set(ch, 2, fctl(0, W - 1, H))), "not the whole canvas")
    m["first_not_at_origin"] = (join(_set(ch, 2, fctl(0, W - 1, H, 1, 0))), "not the whole canvas")
    m["two_fctl_before_idat"] = (join(ch[:3] + [(b"fcTL", fctl(1, W, H))] + ch[3:]), "two fcTL")
    m["dispose_3"] = (join(_set(ch, 4, fctl(1, 6, 5, 2, 3, dispose=3))), "dispose 3")
    m["blend_2"] = (join(_set(ch, 4, fctl(1, 6, 5, 2, 3, blend=2))), "blend 2")
    m["fctl_short"] = (join(_set(ch, 4, ch[4][1][:25])), "fcTL of 25 bytes")
    m["bad_zlib_header"] = (join(_set(ch, 5, ch[5][1][:4] + b"\x79" + ch[5][1][5:])), "zlib header")
    m["no_iend"] = (join(ch[:9]), "no IEND")
    m["no_idat"] = (join(ch[:3] + ch[4:]), "")
    m["truncated_in_fdat"] = (good[:len(join(ch[:6])) - 5], "past the end")
    m["truncated_header"] = (good[:len(join(ch[:7])) + 6], "truncated chunk header")
    m["not_png"] = (b"GIF89a" + good[6:], "signature")
    return m


def unsupported():
    """name -> (file, a word of the reason)"""
    W, H = 19, 14
    u = {}
    u["over_rgba"] = (build(W, H, 6, 8, [frame(pix(H, W, 6, 8, 80)), frame(pix(4, 4, 6, 8, 81), x=1, y=1, blend=1)]), "OVER")
    u["over_grey_alpha"] = (build(W, H, 4, 8, [frame(pix(H, W, 4, 8, 82), blend=1)]), "OVER")
    u["over_palette_trns"] = (build(W, H, 3, 4, [frame(pix(H, W, 3, 4, 83)), frame(pix(4, 4, 3, 4, 84), blend=1)], plte=pfc.palette(4),
                                    trns=b"\0\x80"), "OVER")
    u["trns_grey"] = (build(W, H, 0, 8, [frame(pix(H, W, 0, 8, 85))], trns=b"\0\x05"), "tRNS on colour type 0")
    u["trns_rgb"] = (build(W, H, 2, 8, [frame(pix(H, W, 2, 8, 86)), frame(pix(2, 2, 2, 8, 87))], trns=b"\0\x05\0\x06\0\x07"),
                     "tRNS on colour type 2")
    one = pix(1, 1, 0, 8, 88)
    ch = chunk_list(1, 1, 0, 8, [frame(one), frame(one)])
    u["side_16385"] = (join(_set(_set(ch, 0, struct.pack(">IIBBBBB", 16385, 1, 8, 0, 0, 0, 0)), 2, fctl(0, 16385, 1))), "16384")
    # 65536 frames of one pixel: only the chunk headers count, the frames share one stream
    z = ch[3][1]
    many = ch[:1] + [(b"acTL", struct.pack(">II", 65536, 0)), ch[2], ch[3]]
    for k in range(1, 65536):
        many += [(b"fcTL", fctl(2 * k - 1, 1, 1)), (b"fdAT", struct.pack(">I", 2 * k) + z)]
    u["frames_65536"] = (join(many + [(b"IEND", b"")]), "65535 frames")
    big = chunk_list(1, 1, 0, 8, [frame(one)] * 2)
    u["two_gib"] = (join(_set(_set(big, 0, struct.pack(">IIBBBBB", 16384, 16384, 8, 0, 0, 0, 0)), 2, fctl(0, 16384, 16384))), "2 GiB")
    return u


def corrupt():
    """name -> (file, the VF_PNG_* status the device reports): a frame's stream is damaged behind valid chunk CRCs"""
    W, H, ch = _base()
    c = {}
    raw = zlib.decompress(ch[8][1][4:])
    bad = bytearray(raw)
    bad[0] = 9                                                        # a filter type above 4 in the last frame's first row
    c["bad_filter_last_frame"] = (join(_set(ch, 8, ch[8][1][:4] + zlib.compress(bytes(bad)))), pfc.STATUS["bad filter"])
    c["short_stream_frame1"] = (join(_set(ch, 6, ch[6][1][:-6])), pfc.STATUS["short data"])
    z = bytearray(ch[3][1])
    z[-1] ^= 0x55                                                     # frame 0's Adler-32
    c["bad_adler_frame0"] = (join(_set(ch, 3, bytes(z))), pfc.STATUS["bad Adler-32"])
    c["wrong_size_frame2"] = (join(_set(ch, 7, fctl(4, 4, 5, 10, 9))), pfc.STATUS["bad length"])
    return c


def fixtures():
    """dict(good, malformed, unsupported, corrupt), built once"""
    if not _CACHE:
        good = dict(pillow_written())
        good.update(hand_assembled())
        _CACHE.update(good=good, malformed=malformed(), unsupported=unsupported(), corrupt=corrupt())
    return _CACHE
