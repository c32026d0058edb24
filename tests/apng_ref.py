"""The animated PNG the device encoder writes (vf_apng_encode), as its definition: pure Python on the host.

assemble(png_files, delay, loop): given the N PNG files of a clip's N frames — the ones data.encode_png writes, or any
writer's, as long as they share one IHDR — the APNG is
    signature, frame 0's IHDR,
    acTL (num_frames N, num_plays loop),
    frame 0:      fcTL (sequence number 0, the whole canvas at (0,0), delay / 100 s, dispose NONE, blend SOURCE) and
                  frame 0's IDAT chunks unchanged,
    frame j >= 1: fcTL, then one fdAT per IDAT of frame j's file, in order: its sequence number and the IDAT's payload,
    IEND.
Sequence numbers run 0, 1, 2, ... over fcTL and fdAT together.  Every frame is its own complete zlib stream; nothing is
differenced and no frame is a sub-rectangle.  Chunks other than IHDR, IDAT and IEND are not carried over (encode_png
writes none)."""
import struct
import zlib

SIGNATURE = b"\x89PNG\r\n\x1a\n"
DELAY_DEN = 100                                 # delays are centiseconds, as in the GIF writer


def chunk(ctype, data):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) & 0xFFFFFFFF)


def chunks(png):
    """[(type, payload)] of a PNG file; the CRCs are checked"""
    assert png[:8] == SIGNATURE, "not a PNG file"
    out, at = [], 8
    while at < len(png):
        (n,) = struct.unpack(">I", png[at:at + 4])
        ctype, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        assert len(data) == n and struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(ctype + data) & 0xFFFFFFFF, \
            "chunk %r at %d: truncated or wrong CRC" % (ctype, at)
        out.append((ctype, data))
        at += 12 + n
    assert out and out[0][0] == b"IHDR" and out[-1][0] == b"IEND"
    return out


def fctl(seq, w, h, delay, x=0, y=0, delay_den=DELAY_DEN, dispose=0, blend=0):
    return chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, x, y, delay, delay_den, dispose, blend))


def assemble(png_files, delay=10, loop=0):
    """the APNG of the clip whose frames are png_files, `delay` centiseconds a frame, played `loop` times (0: forever)"""
    n = len(png_files)
    assert 1 <= n <= 65535 and 0 <= delay <= 65535 and 0 <= loop <= 65535
    parsed = [chunks(f) for f in png_files]
    ihdr = parsed[0][0][1]
    w, h = struct.unpack(">II", ihdr[:8])
    out = [SIGNATURE, chunk(b"IHDR", ihdr), chunk(b"acTL", struct.pack(">II", n, loop))]
    seq = 0
    for j, ch in enumerate(parsed):
        assert ch[0][1] == ihdr, "frame %d has another IHDR than frame 0" % j
        idats = [d for t, d in ch if t == b"IDAT"]
        assert idats, "frame %d has no IDAT" % j
        out.append(fctl(seq, w, h, delay))
        seq += 1
        for d in idats:
            if j == 0:
                out.append(chunk(b"IDAT", d))
            else:
                out.append(chunk(b"fdAT", struct.pack(">I", seq) + d))
                seq += 1
    assert seq < 1 << 31
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def read(apng):
    """An independent walk of a file assemble() wrote -> dict(width, height, frames, loop, seqs, delays, streams): the
    sequence numbers in file order, each frame's (delay_num, delay_den) and its zlib stream (data chunks joined)."""
    ch = chunks(apng)
    w, h = struct.unpack(">II", ch[0][1][:8])
    r = dict(width=w, height=h, frames=None, loop=None, seqs=[], delays=[], streams=[], ihdr=ch[0][1])
    for t, d in ch[1:]:
        if t == b"acTL":
            r["frames"], r["loop"] = struct.unpack(">II", d)
        elif t == b"fcTL":
            seq, fw, fh, x, y, dn, dd, dispose, blend = struct.unpack(">IIIIIHHBB", d)
            assert (fw, fh, x, y, dispose, blend) == (w, h, 0, 0, 0, 0)
            r["seqs"].append(seq)
            r["delays"].append((dn, dd))
            r["streams"].append(b"")
        elif t == b"IDAT":
            r["streams"][-1] += d
        elif t == b"fdAT":
            r["seqs"].append(struct.unpack(">I", d[:4])[0])
            r["streams"][-1] += d[4:]
    return r
