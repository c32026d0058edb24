"""Host definition of the device GIF decoder (vf_gif_decode.hip).  NumPy and the standard library only; all
integer.  `decode(data)` is the rule; the device equals it byte for byte, and Pillow agrees with it on the class of files
where Pillow's own result does not depend on its background fill (tests/gif_decode_cases.py names that class).

Container: `GIF87a` or `GIF89a`; logical screen descriptor; a global colour table of 2 << (packed & 7) entries when packed &
0x80; then any sequence of
  21 F9 04 pp dd dd tt 00   graphic control extension: disposal = (pp >> 2) & 7, transparent index tt when pp & 1, delay dd
                            in centiseconds; it belongs to the next image and is used up by it;
  21 FF 0B NETSCAPE2.0 03 01 ll ll ...   the loop count ll; other application extensions, comments (21 FE), plain text
                            (21 01) and every other 21 xx are skipped sub-block by sub-block;
  2C x x y y w w h h pp     image descriptor: local table of 2 << (pp & 7) entries when pp & 0x80, interlaced when pp & 0x40;
                            then the LZW minimum code size and the data sub-blocks up to the terminator 00;
  3B                        the trailer: the file ends here, whatever follows.
Malformed (GifMalformed): a bad signature, a file that ends before its trailer, a screen or rectangle side of 0, a
rectangle that leaves the screen, a frame with neither a local nor a global table, a minimum code size outside 2 .. 8, an
unknown block introducer, no frame at all.  Unsupported (parse()["supported"] False, with a reason): a side above 16384,
more than 65535 frames, frames * H * W * 4 of 2 GiB or more, frame rectangles above 2^28 pixels, image data of a frame above
2^28 bytes.

LZW (`unlzw`): Clear = 1 << m, EOI = Clear + 1, first free code Clear + 2, width m + 1, codes LSB first.  The stream starts
in the state behind a Clear whether or not one stands there.  A Clear resets; the first code behind it must be a root
(<= EOI counts: EOI ends the data).  Every later code c must be <= the next free code n; it adds entry n = previous string
+ first index of c's string (c == n: the previous string + its own first index) while n < 4096, after which the width grows
when n reaches 1 << width, up to 12; with 4096 entries nothing is added and the width stays 12 until a Clear.  Decoding
stops when w * h indices are there; what follows is not read.  Status of a frame: BAD_CODE (a code above n, or a first code
behind a Clear above EOI), SHORT_DATA (EOI, or fewer bits left than the code's width, before the rectangle is full).

Interlace: the stream's rows are rows 0, 8, 16, ...; then 4, 12, ...; then 2, 6, 10, ...; then 1, 3, 5, ... of the rectangle.

Compositing: the canvas is RGBA, H x W, all (0,0,0,0).  For frame k: remember the canvas if disposal is 3; every index of
the rectangle that is not the transparent one becomes (table[index], 255); the canvas is output frame k; then disposal 2
sets the rectangle to (0,0,0,0), 3 puts the remembered canvas back, 0, 1 and 4 .. 7 change nothing.  RGB output is the three
colour planes.  An index that is painted and is not below the table's size gives BAD_INDEX.

A file's status is the largest of its frames' LZW status words; BAD_INDEX is looked for only when all of them are OK.
"""
import struct

import numpy as np

OK, BAD_CODE, SHORT_DATA, BAD_INDEX = 0, 1, 2, 3
STATUS_WORD = {1: "bad code", 2: "short data", 3: "bad colour index"}
MAX_SIDE, MAX_FRAMES = 16384, 65535
FRAME_KEYS = ("delay", "disposal", "x", "y", "w", "h", "interlace", "transparency", "table_size", "local_table", "min_code_size",
              "data_bytes")


class GifMalformed(ValueError):
    pass


def parse(data):
    """bytes -> dict(width, height, frames, loop, global_table_size, version, supported, reason, frame_info, tables, streams):
    frame_info a list of dicts of FRAME_KEYS, tables the active uint8 [size][3] table of every frame, streams the
    concatenated data sub-blocks of every frame."""
    d = bytes(data)
    n = len(d)

    def need(cond, what):
        if not cond:
            raise GifMalformed(what)
    need(d[:6] in (b"GIF87a", b"GIF89a"), "bad signature")
    need(n >= 13, "truncated logical screen descriptor")
    W, H, packed = struct.unpack("<HHB", d[6:11])
    need(W >= 1 and H >= 1, "empty logical screen")
    pos, gtable = 13, None
    if packed & 0x80:
        size = 2 << (packed & 7)
        need(pos + 3 * size <= n, "truncated global colour table")
        gtable = np.frombuffer(d[pos:pos + 3 * size], np.uint8).reshape(size, 3)
        pos += 3 * size

    def blocks():
        nonlocal pos
        out = bytearray()
        while True:
            need(pos < n, "sub-blocks run past the end of the file")
            ln = d[pos]
            pos += 1
            if ln == 0:
                return bytes(out)
            need(pos + ln <= n, "sub-blocks run past the end of the file")
            out += d[pos:pos + ln]
            pos += ln
    loop, gce = -1, (0, -1, 0)
    info, tables, streams = [], [], []
    while True:
        need(pos < n, "no trailer")
        b = d[pos]
        pos += 1
        if b == 0x3B:
            break
        if b == 0x21:
            need(pos < n, "truncated extension")
            label = d[pos]
            pos += 1
            if label == 0xF9 and pos + 6 <= n and d[pos] == 4 and d[pos + 5] == 0:
                pp, delay, tt = d[pos + 1], d[pos + 2] | d[pos + 3] << 8, d[pos + 4]
                gce = ((pp >> 2) & 7, tt if pp & 1 else -1, delay)
                pos += 6
                continue
            if label == 0xFF and d[pos:pos + 12] == b"\x0bNETSCAPE2.0" and pos + 16 <= n and d[pos + 12] == 3 and d[pos + 13] == 1:
                loop = d[pos + 14] | d[pos + 15] << 8
            blocks()
            continue
        need(b == 0x2C, "unknown block introducer %d" % b)
        need(pos + 9 <= n, "truncated image descriptor")
        x, y, w, h, pp = struct.unpack("<HHHHB", d[pos:pos + 9])
        pos += 9
        need(w >= 1 and h >= 1 and x + w <= W and y + h <= H, "frame %d: the rectangle leaves the screen" % len(info))
        if pp & 0x80:
            size = 2 << (pp & 7)
            need(pos + 3 * size <= n, "truncated local colour table")
            table = np.frombuffer(d[pos:pos + 3 * size], np.uint8).reshape(size, 3)
            pos += 3 * size
        else:
            need(gtable is not None, "frame %d: no local colour table and no global one" % len(info))
            table = gtable
        need(pos < n, "no image data")
        m = d[pos]
        pos += 1
        need(2 <= m <= 8, "frame %d: LZW minimum code size %d" % (len(info), m))
        stream = blocks()
        info.append(dict(delay=gce[2], disposal=gce[0], x=x, y=y, w=w, h=h, interlace=(pp >> 6) & 1, transparency=gce[1],
                         table_size=len(table), local_table=(pp >> 7) & 1, min_code_size=m, data_bytes=len(stream)))
        tables.append(table)
        streams.append(stream)
        gce = (0, -1, 0)
    need(info, "no frame")
    why = ""
    if W > MAX_SIDE or H > MAX_SIDE:
        why = "larger than 16384 per side"
    elif len(info) > MAX_FRAMES:
        why = "more than 65535 frames"
    elif len(info) * W * H * 4 >= 1 << 31:
        why = "decoded frames of 2 GiB or more"
    elif sum(f["w"] * f["h"] for f in info) > 1 << 28:
        why = "frame rectangles above 256 Mi pixels"
    elif max(f["data_bytes"] for f in info) > 1 << 28:
        why = "a frame's image data above 256 MiB"
    return dict(width=W, height=H, frames=len(info), loop=loop, global_table_size=0 if gtable is None else len(gtable),
                version=87 if d[4:5] == b"7" else 89, supported=not why, reason=why, frame_info=info, tables=tables, streams=streams)


def unlzw(stream, m, npix):
    """-> (npix indices as uint8, missing ones 0; status)"""
    clear, eoi = 1 << m, (1 << m) + 1
    nbits = 8 * len(stream)
    acc = int.from_bytes(stream, "little")
    pos, out = 0, []
    table, width, prev = {}, m + 1, None              # table: code -> list; roots are implicit
    nxt = eoi + 1
    status = OK
    while len(out) < npix:
        if pos + width > nbits:
            status = SHORT_DATA
            break
        c = (acc >> pos) & ((1 << width) - 1)
        pos += width
        if c == clear:
            table, width, prev, nxt = {}, m + 1, None, eoi + 1
            continue
        if c == eoi:
            status = SHORT_DATA
            break
        if prev is None:
            if c > eoi:
                status = BAD_CODE
                break
            s = [c]
        else:
            if c > nxt:
                status = BAD_CODE
                break
            if c < clear:
                s = [c]
            elif c < nxt:
                s = table[c]
            else:
                s = prev + [prev[0]]
            if nxt < 4096:
                table[nxt] = prev + [s[0]]
                nxt += 1
                if nxt == 1 << width and width < 12:
                    width += 1
        out += s
        prev = s
    idx = np.zeros(npix, np.uint8)
    got = min(len(out), npix)
    idx[:got] = out[:got]
    return idx, status


def lace_order(h):
    """display row of every row of the stream of an interlaced frame"""
    return [r for start, step in ((0, 8), (4, 8), (2, 4), (1, 2)) for r in range(start, h, step)]


def decode(data, alpha=False):
    """bytes -> (frames uint8 N x H x W x (4 if alpha else 3), status, parse(data)).  With a non-zero status the frames are
    not defined (the device's are not compared)."""
    meta = parse(data)
    W, H, N = meta["width"], meta["height"], meta["frames"]
    planes, status = [], OK
    for f, stream in zip(meta["frame_info"], meta["streams"]):
        idx, st = unlzw(stream, f["min_code_size"], f["w"] * f["h"])
        status = max(status, st)
        idx = idx.reshape(f["h"], f["w"])
        if f["interlace"]:
            rows = np.empty_like(idx)
            rows[lace_order(f["h"])] = idx
            idx = rows
        planes.append(idx)
    canvas = np.zeros((H, W, 4), np.uint8)
    out = np.zeros((N, H, W, 4), np.uint8)
    bad_index = False
    for k, (f, table, idx) in enumerate(zip(meta["frame_info"], meta["tables"], planes)):
        saved = canvas.copy() if f["disposal"] == 3 else None
        y, x, h, w = f["y"], f["x"], f["h"], f["w"]
        paint = idx != f["transparency"]
        oob = paint & (idx >= len(table))
        bad_index |= bool(oob.any())
        paint &= ~oob
        rect = canvas[y:y + h, x:x + w]
        rect[paint, :3] = table[idx[paint]]
        rect[paint, 3] = 255
        out[k] = canvas
        if f["disposal"] == 2:
            canvas[y:y + h, x:x + w] = 0
        elif f["disposal"] == 3:
            canvas = saved
    if status == OK and bad_index:
        status = BAD_INDEX
    return (out if alpha else np.ascontiguousarray(out[..., :3])), status, meta
