"""Host restatement of the animated-PNG decode rule (vf_apng_inspect / vf_apng_decode), built on
png_full_ref: NumPy on the host, the definition the device decoder is compared with; tests/test_apng_decode_ref.py pins
it against Pillow.

Frames.  N is acTL.num_frames, which must be the number of fcTL chunks.  Frame k's pixels are the zlib stream of its data
chunks — the IDATs when its fcTL precedes them, otherwise its fdATs without their 4-byte sequence numbers — decoded under
the full PNG rule as an image of the fcTL's width x height with the IHDR's depth, colour type and interlace and the
file's PLTE / tRNS (a 16-bit sample gives its high byte).  A default image with no fcTL in front of it is not a frame.  A
PNG without acTL is a clip of one frame, the image; fcTL and fdAT chunks in such a file are ancillary chunks nobody reads.

Canvas.  The IHDR's size, transparent black at the start.  Blend SOURCE replaces the frame's rectangle, alpha included
(OVER in a file without alpha is the same thing; with alpha it is unsupported).  Output frame k is the canvas after frame
k was rendered.  Then dispose NONE (0) leaves the canvas, BACKGROUND (1) clears the rectangle to transparent black,
PREVIOUS (2) restores what was there before the frame; on the first frame PREVIOUS is BACKGROUND.  Grey is replicated to
RGB, files without alpha paint alpha 255, a pixel nothing has painted is (0,0,0,0).

Sequence numbers run 0, 1, 2, ... over fcTL and fdAT in file order.  CRCs are checked on IHDR, PLTE, tRNS, IDAT, IEND,
acTL, fcTL and fdAT."""
import struct
import zlib

import numpy as np

import png_full_ref
from png_load_ref import PngError, PngUnsupported

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHECKED = (b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND", b"acTL", b"fcTL", b"fdAT")
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
FRAME_KEYS = ("x", "y", "w", "h", "delay_num", "delay_den", "dispose", "blend", "data_bytes")
MAX_SIDE, MAX_FRAMES = 16384, 65535


class ApngError(PngError):
    """malformed"""


class ApngUnsupported(PngUnsupported):
    """well-formed, but not taken by the device decoder"""


def _chunk(ctype, data):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) & 0xFFFFFFFF)


def parse(data):
    """-> dict(width, height, bit_depth, color_type, interlace, channels, frames, num_plays (-1 without acTL), animated,
    default_is_frame, supported, reason, plte (bytes or None), trns (bytes or None), frame_info: per frame a dict of
    FRAME_KEYS and `data`, its zlib stream).  ApngError for a malformed file."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise ApngError("not a PNG file (bad signature)")
    pos, n = 8, len(data)
    ihdr = plte = trns = None
    animated, num_frames, num_plays = False, 0, -1
    seq, frames, idat, idat_frame = 0, [], [], None
    seen_idat = idat_done = iend = over = False
    while pos < n:
        if pos + 12 > n:
            raise ApngError("truncated chunk header at byte %d" % pos)
        (L,) = struct.unpack(">I", data[pos:pos + 4])
        ty = data[pos + 4:pos + 8]
        if pos + 12 + L > n:
            raise ApngError("chunk %r at byte %d runs past the end of the file" % (ty, pos))
        body = data[pos + 8:pos + 8 + L]
        if (ihdr is None) != (ty == b"IHDR"):
            raise ApngError("IHDR is not the first chunk" if ihdr is None else "more than one IHDR")
        if ty in CHECKED and zlib.crc32(ty + body) & 0xFFFFFFFF != struct.unpack(">I", data[pos + 8 + L:pos + 12 + L])[0]:
            raise ApngError("wrong CRC on chunk %s at byte %d" % (ty.decode(), pos))
        if seen_idat and ty != b"IDAT":
            idat_done = True
        if ty == b"IHDR":
            if L != 13:
                raise ApngError("IHDR of %d bytes" % L)
            W, H, depth, ct, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            ok = depth in (1, 2, 4, 8, 16) and (ct == 0 or (ct == 3 and depth <= 8) or (ct in (2, 4, 6) and depth >= 8))
            if not (1 <= W <= 0x7fffffff and 1 <= H <= 0x7fffffff and ok and comp == 0 and filt == 0 and lace <= 1):
                raise ApngError("illegal IHDR")
            ihdr = body
        elif ty == b"PLTE":
            if seen_idat or plte is not None or L == 0 or L % 3 or L > 768 or ct in (0, 4) or (ct == 3 and L // 3 > 1 << depth):
                raise ApngError("illegal PLTE")
            plte = body
        elif ty == b"tRNS":
            ok = not seen_idat and trns is None and ((ct == 3 and plte is not None and 1 <= L <= len(plte) // 3) or
                                                     (ct == 0 and L == 2) or (ct == 2 and L == 6))
            if not ok:
                raise ApngError("illegal tRNS")
            trns = body
        elif ty == b"acTL":
            if animated:
                raise ApngError("a second acTL at byte %d" % pos)
            if seen_idat:
                raise ApngError("acTL after IDAT at byte %d" % pos)
            if L != 8:
                raise ApngError("acTL of %d bytes" % L)
            animated = True
            num_frames, num_plays = struct.unpack(">II", body)
            if num_frames == 0:
                raise ApngError("acTL: num_frames is 0")
        elif ty == b"fcTL" and animated:
            if L != 26:
                raise ApngError("fcTL of %d bytes" % L)
            s, w, h, x, y, dn, dd, dispose, blend = struct.unpack(">IIIIIHHBB", body)
            if s != seq:
                raise ApngError("fcTL at byte %d has sequence number %d, %d is due" % (pos, s, seq))
            seq += 1
            if idat_frame is not None and not seen_idat:
                raise ApngError("two fcTL chunks in front of IDAT")
            who = "frame %d" % len(frames)
            if w == 0 or h == 0:
                raise ApngError("%s is %dx%d" % (who, w, h))
            if x + w > W or y + h > H:
                raise ApngError("%s: %dx%d at (%d,%d) leaves the %dx%d canvas" % (who, w, h, x, y, W, H))
            if dispose > 2:
                raise ApngError("%s: dispose %d" % (who, dispose))
            if blend > 1:
                raise ApngError("%s: blend %d" % (who, blend))
            if not seen_idat:
                if (x, y, w, h) != (0, 0, W, H):
                    raise ApngError("the fcTL in front of IDAT is not the whole canvas at (0,0)")
                idat_frame = len(frames)
            over = over or blend == 1
            frames.append(dict(x=x, y=y, w=w, h=h, delay_num=dn, delay_den=dd, dispose=dispose, blend=blend, parts=[],
                               in_idat=not seen_idat))
        elif ty == b"fdAT" and animated:
            if not frames:
                raise ApngError("fdAT at byte %d before the first fcTL" % pos)
            if L < 4:
                raise ApngError("fdAT of %d bytes at byte %d" % (L, pos))
            (s,) = struct.unpack(">I", body[:4])
            if s != seq:
                raise ApngError("fdAT at byte %d has sequence number %d, %d is due" % (pos, s, seq))
            seq += 1
            if frames[-1]["in_idat"]:
                raise ApngError("fdAT at byte %d in the frame that the IDAT chunks hold" % pos)
            frames[-1]["parts"].append(body[4:])
        elif ty == b"IDAT":
            if idat_done:
                raise ApngError("IDAT chunks are not consecutive")
            if ct == 3 and plte is None:
                raise ApngError("no PLTE before IDAT for colour type 3")
            seen_idat = True
            idat.append(body)
        elif ty == b"IEND":
            if L:
                raise ApngError("IEND of %d bytes" % L)
            iend = True
            break
        elif not ty[0] & 0x20:
            raise ApngError("unknown critical chunk %r" % ty)
        pos += 12 + L
    if ihdr is None:
        raise ApngError("no IHDR")
    if not iend:
        raise ApngError("no IEND chunk")
    if not seen_idat:
        raise ApngError("no IDAT chunk")
    if not animated:
        frames = [dict(x=0, y=0, w=W, h=H, delay_num=0, delay_den=0, dispose=0, blend=0, parts=idat)]
    else:
        if len(frames) != num_frames:
            raise ApngError("%d fcTL chunks, acTL says %d frames" % (len(frames), num_frames))
        if idat_frame == 0:
            frames[0]["parts"] = idat
    for k, f in enumerate(frames):
        f["data"] = b"".join(f.pop("parts"))
        f.pop("in_idat", None)
        f["data_bytes"] = len(f["data"])
        if not f["data"]:
            raise ApngError("frame %d has no data" % k)
        z = f["data"][:2]
        if len(z) < 2 or (z[0] & 15) != 8 or (z[0] >> 4) > 7 or (z[1] & 0x20) or (z[0] * 256 + z[1]) % 31:
            raise ApngError("frame %d: bad zlib header" % k)
    fc = (4 if trns is not None else 3) if ct == 3 else SAMPLES[ct] + (1 if ct in (0, 2) and trns is not None else 0)
    why = ""
    if trns is not None and ct != 3:
        why = "tRNS on colour type %d (alpha from a colour key)" % ct
    elif over and (ct in (4, 6) or trns is not None):
        why = "blend OVER in a file that carries alpha"
    elif max(W, H) > MAX_SIDE:
        why = "larger than 16384 per side"
    elif len(frames) > MAX_FRAMES:
        why = "more than 65535 frames"
    elif len(frames) * W * H * 4 >= 1 << 31:
        why = "2 GiB or more of RGBA frames"
    else:
        for k, f in enumerate(frames):
            inflated = sum(h * (1 + rb) for _, h, rb in png_full_ref.passes(f["w"], f["h"], SAMPLES[ct], depth, lace))
            if f["data_bytes"] > 1 << 28 or inflated >= 1 << 31:
                why = "frame %d: too large for the full rule" % k
                break
    return dict(width=W, height=H, bit_depth=depth, color_type=ct, interlace=lace, channels=fc, frames=len(frames),
                num_plays=num_plays, animated=animated, default_is_frame=not animated or idat_frame == 0, supported=not why,
                reason=why, plte=plte, trns=trns, frame_info=frames)


def frame_png(d, k):
    """frame k of a parsed file as a PNG file of its own: what the full rule decodes"""
    f = d["frame_info"][k]
    out = SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", f["w"], f["h"], d["bit_depth"], d["color_type"], 0, 0, d["interlace"]))
    if d["plte"] is not None:
        out += _chunk(b"PLTE", d["plte"])
    if d["trns"] is not None:
        out += _chunk(b"tRNS", d["trns"])
    return out + _chunk(b"IDAT", f["data"]) + _chunk(b"IEND", b"")


def rgba(px):
    """h x w x (1, 2, 3, 4) -> h x w x 4: grey replicated, alpha 255 where there is none"""
    c = px.shape[2]
    col = np.repeat(px[..., :1], 3, axis=2) if c <= 2 else px[..., :3]
    al = px[..., -1:] if c in (2, 4) else np.full(px.shape[:2] + (1,), 255, np.uint8)
    return np.concatenate([col, al], axis=2)


def decode(data, alpha=False):
    """-> uint8 N x H x W x (4 if alpha else 3): the canvas after every frame.  ApngError for a malformed file or a corrupt
    frame stream (PngError from the full rule), ApngUnsupported for one the device decoder does not take."""
    d = parse(data)
    if not d["supported"]:
        raise ApngUnsupported(d["reason"])
    W, H, N = d["width"], d["height"], d["frames"]
    canvas = np.zeros((H, W, 4), np.uint8)
    out = np.zeros((N, H, W, 4), np.uint8)
    for k, f in enumerate(d["frame_info"]):
        px = rgba(png_full_ref.load(frame_png(d, k)))
        x, y, w, h = f["x"], f["y"], f["w"], f["h"]
        before = canvas[y:y + h, x:x + w].copy()
        canvas[y:y + h, x:x + w] = px                       # SOURCE (OVER is only taken where it is the same)
        out[k] = canvas
        if f["dispose"] == 1 or (f["dispose"] == 2 and k == 0):
            canvas[y:y + h, x:x + w] = 0
        elif f["dispose"] == 2:
            canvas[y:y + h, x:x + w] = before
    return out if alpha else np.ascontiguousarray(out[..., :3])


def metadata(data):
    """what vf_apng_inspect reports: (info dict without the byte fields, [FRAME_KEYS rows])"""
    d = parse(data)
    info = {k: d[k] for k in ("width", "height", "bit_depth", "color_type", "interlace", "channels", "frames", "num_plays",
                              "supported", "animated", "default_is_frame")}
    info["palette_entries"] = len(d["plte"]) // 3 if d["plte"] is not None else 0
    return info, [[f[k] for k in FRAME_KEYS] for f in d["frame_info"]]
