"""Batch preparation on the device — the loader side of the hot path.

The reference prepares every sample on the host, inside the loader threads (datavid/donkey_folder.lua:135-189) or at
the top of the closure (train.lua:284-298), and then copies the batch to the GPU.  Here the host only decodes and
draws the random numbers; cropping, masking, flipping, the [0,1] -> [-1,1] map and the NCHW -> NHWC conversion are one
kernel per sample, writing straight into the batch buffers the closures read (`vf_clip_prepare`, `vf_center_prepare`).
The resize before them — Torch7's image.scale in the loaders' loadImage / loadContImages — is on the device too
(vf_image.hip): `image_scale`, `ImageBatcher` (train.lua's loader, one fused launch per image) and
`ClipBatcher.add_frames` take decoded frames, and `PatchArrayBatcher` (train_wholeim_input.lua's loader: the 3 x 3
patch array of datavid/donkey_wholeim.lua, one fused launch per frame, `vf_patch_array_prepare`) does the same for the
widest net.  The decode before them — image.load, libjpeg underneath — is on the
device as well (vf_jpeg.hip): `decode_jpeg` turns a batch of baseline JPEG files (with progressive=True
progressive ones too) into those frames, byte for byte what libjpeg gives, so the host only reads the
files and draws the random numbers.
"""
import math
import os
import re

import numpy as np
import torch

from ._lib import VfError
from .backend import (GIF_STATUS, JPEG_STATUS, METRIC_COLUMNS, PNG_STATUS, apng_inspect, get_backend, gif_inspect, jpeg_inspect,
                      jpeg_inspect_layouts, jpeg_scans_inspect, nhwc_empty, png_inspect, png_inspect_full)

CENTER_FILL = (117.0, 104.0, 123.0)      # train.lua:287-289


# ------------------------------------------------------------------------------------------------ JPEG
def _file_bytes(item):
    """bytes of one image file (JPEG, PNG) given as bytes / bytearray / memoryview, a uint8 array or tensor, or a path."""
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    if isinstance(item, (str, os.PathLike)):
        with open(item, "rb") as fh:
            return fh.read()
    if isinstance(item, torch.Tensor):
        item = item.cpu().numpy()
    a = np.asarray(item)
    assert a.dtype == np.uint8, "a file as an array is uint8"
    return a.tobytes()


def _stacked(out, buf, dev):
    """stack=True: the images of one shape as one N x H x W x C tensor — a view of the decoder's buffer `buf` when all of
    them came from it (dev names them all: they lie back to back), else a copy."""
    shapes = {tuple(t.shape) for t in out}
    assert len(shapes) == 1, "stack=True needs images of one shape, got %s" % sorted(shapes)
    if buf is not None and len(dev) == len(out):
        return buf[:len(out) * out[0].numel()].view(len(out), *out[0].shape)
    return torch.stack(out)


def _decode_files(who, files, channels, fallback, inspect, refuse, run, status_names, corrupt_text, shape_of, stack):
    """The batch decoders' host side.  inspect(file) -> its info, or ValueError; refuse(info, channels) -> why a supported
    file goes to the fallback after all, or None; run(files, infos) -> (buffer, offsets, status) of the device decode;
    shape_of(info) -> the image's H, W, C.  Files the device decoder does not take go to fallback(bytes) or raise
    ValueError; every error names the item by its place in `files`."""
    B = get_backend()
    infos, dev, out = [], [], [None] * len(files)
    for i, f in enumerate(files):
        try:
            info = inspect(f)
        except ValueError as e:
            raise ValueError("%s: item %d: %s" % (who, i, e)) from None
        why = refuse(info, channels) if info["supported"] else info["reason"]
        if why is not None:
            if fallback is None:
                raise ValueError("%s: item %d is not supported by the device decoder: %s" % (who, i, why))
            img = torch.as_tensor(np.ascontiguousarray(fallback(f)))
            if img.dim() == 2:
                img = img.unsqueeze(-1)
            assert img.dtype == torch.uint8 and img.dim() == 3 and (channels is None or img.shape[2] == channels), \
                "fallback returns uint8 H x W x %s, got %s %s" % (channels or "C", img.dtype, tuple(img.shape))
            out[i] = B.from_host(img).contiguous()
            continue
        infos.append(info)
        dev.append(i)
    buf = None
    if dev:
        try:
            buf, offs, status = run([files[i] for i in dev], infos)
        except VfError as e:   # found on the host while the batch was planned: nothing was launched
            m = re.search(r"image (\d+)", str(e))
            if m is None:
                raise
            raise ValueError("%s: item %d: %s" % (who, dev[int(m.group(1))], e)) from None
        st = status.cpu().tolist()
        for j, i in enumerate(dev):
            if st[j] != 0:
                raise ValueError("%s: item %d: %s (%s)" % (who, i, corrupt_text, status_names.get(st[j], st[j])))
            out[i] = buf[offs[j]:offs[j + 1]].view(*shape_of(infos[j]))
    return _stacked(out, buf, dev) if stack else out


def jpeg_info(item, layouts=False):
    """The host-side inspection of one JPEG file (no GPU): dict(width, height, components, h_samp, v_samp,
    restart_interval, scan_begin, scan_end, supported, sof, segments, precision, reason).  ValueError if its headers
    cannot be parsed (truncated, no SOS).  layouts=True: the walk of the whole file under decode_jpeg's layouts=True
    instead: dict(width, height, components, sampling, colour, scans, supported, sof, precision, levels, blocks,
    blocks_per_mcu, reason)."""
    return jpeg_inspect_layouts(_file_bytes(item)) if layouts else jpeg_inspect(_file_bytes(item))


def jpeg_scans(item):
    """The scans of one progressive JPEG file, from the host-side walk of the whole file (no GPU): a list of
    dict(components, Ss, Se, Ah, Al, restart_interval, begin, end, segments, level, units) in file order — libjpeg's
    default script gives 10 for a colour file and 6 for a grey one.  Empty for a file whose headers already rule it out
    (backend.jpeg_scans_inspect says why).  ValueError if the file is malformed."""
    return jpeg_scans_inspect(_file_bytes(item))["scans"]


def _inspect_jpeg_any(f):
    """jpeg_inspect of the headers; for a progressive (SOF2) file the walk of its scans instead, marked progressive."""
    info = jpeg_inspect(f, walk=False)
    if info["sof"] == 0xC2:
        info = dict(jpeg_scans_inspect(f), progressive=True)
    return info


def _run_jpeg_mixed(B, files, infos, channels, subseq_bytes):
    """Baseline and progressive files into one buffer, in the files' order: one device call per kind."""
    n = len(files)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([s["height"] * s["width"] * channels for s in infos])
    buf = torch.empty(max(int(offs[-1]), 1), dtype=torch.uint8, device=B.device)
    parts, order = [], []
    for prog in (False, True):
        idx = [j for j, s in enumerate(infos) if bool(s.get("progressive")) == prog]
        if not idx:
            continue
        sub, sub_infos, into = [files[j] for j in idx], [infos[j] for j in idx], (buf, offs[idx])
        try:
            got = (B.jpeg_prog_decode if prog else B.jpeg_decode)(sub, channels, subseq_bytes, sub_infos, into)
        except VfError as e:   # the image's number in `files`
            raise VfError(re.sub(r"image (\d+)", lambda m: "image %d" % idx[int(m.group(1))], str(e), count=1)) from None
        parts.append(got[2])
        order += idx
    place = torch.as_tensor(np.argsort(order), device=B.device)
    return buf, offs, torch.cat(parts).index_select(0, place)


def decode_jpeg(items, channels=3, stack=False, fallback=None, subseq_bytes=256, progressive=False, layouts=False):
    """image.load(path, channels) of a batch of JPEG files, decoded on the device in one pass (vf_jpeg_decode):
    uint8 H x W x channels device tensors, byte for byte what libjpeg's default decompression gives (Pillow's
    decode; Torch7's image.load followed by :mul(255)).  channels 3 replicates grayscale files; 1 takes grayscale
    files only.

    items: bytes, uint8 arrays or paths.  Returns a list of views into one device buffer, or with stack=True one
    N x H x W x channels tensor (all sizes must match; ClipBatcher.add_frames takes it).  Files the device decoder does
    not support (progressive, arithmetic, 12-bit, CMYK / RGB, 4:4:0, 4:1:1, multi-scan) go to fallback(bytes), which
    returns the decoded uint8 H x W x channels image; without it they raise ValueError naming the item and why.  A
    malformed file raises ValueError naming the item (before anything is launched when the headers or the restart
    markers show it; once the stream has synchronised when the entropy-coded data is corrupt).

    progressive=True also decodes progressive files on the device (vf_jpeg_prog_decode): SOF2,
    Huffman-coded, 8-bit, grey or YCbCr in 4:4:4 / 4:2:2 / 4:2:0, with or without restart intervals, up to 64 scans
    whose progression is orderly and complete — what Pillow, libjpeg, mozjpeg and "save for web" write.  Baseline and
    progressive items may be mixed; the results come back in item order as views of one buffer.  A progressive file with
    an incomplete progression or one out of order (libjpeg block-smooths those: no one result), arithmetic coding, 12
    bits, CMYK, 4:4:0 or 4:1:1 still goes to the fallback or raises with that reason; a scan with impossible parameters
    or an undefined Huffman table is malformed.  Opt-in, and measured: the time goes to the refinement
    scans, which one lane per restart segment walks in order.  On files without restart intervals the device is NOT
    ahead of Pillow on 16 host threads (64 files of 537 x 936: about 430 ms against 40 ms; 256 of 360 x 480: 163 ms
    against 66 ms); on files with a restart interval of one MCU row it is (23 ms against 27 ms; 25 ms against 61 ms).
    The default leaves every result and error as it was.

    layouts=True (implies progressive=True) decodes on the device, in one call (vf_jpeg_decode_layouts),
    every 8-bit Huffman-coded SOF0 / SOF1 / SOF2 file of 1 or 3 components that libjpeg decodes without comment: any
    sampling factors 1..4 whose ratios to the largest are whole numbers with at most 10 blocks in the MCU (4:4:0, 4:1:1,
    4:1:0, subsampled luma, ...), RGB files (Adobe transform 0, or ids 'R','G','B' without a JFIF or Adobe marker), and
    sequential files of several scans (one per component, Y | CbCr, ...; SOF1 with table slots 0..3).  Such files may
    be mixed with the other kinds; the results come back in item order as views of one buffer.  What still goes to the
    fallback or raises with its reason: 4 components, arithmetic coding, 12 bits, lossless and hierarchical files, sides
    above 16384, fractional sampling ratios, a component in no scan; a component in two scans is malformed.  Measured
    (64 files of 537 x 936 / 256 of 360 x 480 against Pillow on 16 threads): 4:4:0 files 5.1 ms against 25 ms
    / 7.7 ms against 71 ms, RGB 4:4:4 files 16 ms against 35 ms / 23 ms against 62 ms, both bound by the host call, which
    walks every file twice; ordinary 4:2:0 files 2.9 / 3.1 ms, where the default entry takes 3.0 / 2.9 ms.  The default
    leaves every result and error as it was."""
    assert channels in (1, 3), "channels is 1 or 3"
    B = get_backend()
    refuse = lambda info, ch: "YCbCr file with channels=1" if ch == 1 and info["components"] != 1 else None
    shape_of = lambda info: (info["height"], info["width"], channels)
    files = [_file_bytes(it) for it in items]
    if layouts:
        return _decode_files("decode_jpeg", files, channels, fallback, jpeg_inspect_layouts,
                             lambda info, ch: "%s file with channels=1" % info["colour"] if ch == 1 and info["components"] != 1 else None,
                             lambda fs, infos: B.jpeg_decode_layouts(fs, channels, subseq_bytes, infos)[:3], JPEG_STATUS,
                             "corrupt entropy-coded data", shape_of, stack)
    if progressive:
        return _decode_files("decode_jpeg", files, channels, fallback, _inspect_jpeg_any, refuse,
                             lambda fs, infos: _run_jpeg_mixed(B, fs, infos, channels, subseq_bytes), JPEG_STATUS,
                             "corrupt entropy-coded data", shape_of, stack)
    return _decode_files(
        "decode_jpeg", files, channels, fallback,
        lambda f: jpeg_inspect(f, walk=False),   # the headers say whether it is supported; the decode walks the scan
        refuse, lambda files, infos: B.jpeg_decode(files, channels, subseq_bytes, infos)[:3], JPEG_STATUS,
        "corrupt entropy-coded data", shape_of, stack)


# ------------------------------------------------------------------------------------------ PNG decode
def png_info(item, full=False):
    """The host-side inspection of one PNG file (no GPU): dict(width, height, bit_depth, color_type, interlace, channels,
    idat_bytes, idat_chunks, palette_entries, trns_entries, supported, inflated_bytes, reason).  ValueError if the file
    is malformed (signature, chunk order, CRC, zlib header).  full=True: supported, reason and inflated_bytes are those of
    the full rule (decode_png's full=True), and passes holds seven (width, height, rowbytes): the Adam7 passes, zeros for
    an absent one; a file without interlace is one pass, the first."""
    return (png_inspect_full if full else png_inspect)(_file_bytes(item))


def decode_png(items, channels=None, stack=False, fallback=None, dtype="uint8", full=False):
    """image.load(path[, channels]) of a batch of PNG files, decoded on the device in one pass (vf_png_decode): uint8
    H x W x C device tensors holding the bytes libpng gives with grey below 8 bits and palettes expanded (Torch7's
    image.load followed by :mul(255)).  channels None keeps the file's own (1 grey, 2 grey+alpha, 3 RGB or palette, 4 RGBA
    or palette with tRNS); 3 replicates grey, takes the grey of grey+alpha and drops the alpha of RGBA; 1 takes grey and
    grey+alpha files only.  dtype "float" divides by 255 in float32 (image.load(path, nc, 'float')).

    items: bytes, uint8 arrays or paths.  Returns a list of views into one device buffer, or with stack=True one
    N x H x W x C tensor (all shapes must match).  Files the device decoder does not support (16-bit samples, Adam7
    interlace, a colour file with channels=1, tRNS on a grey or RGB file with channels=None) go to fallback(bytes), which
    returns the decoded uint8 H x W x C image; without it they raise ValueError naming the item and why.  A malformed
    file raises ValueError naming the item before anything is launched; a corrupt stream raises it, with the status,
    once the stream has synchronised.

    full=True also decodes Adam7-interlaced files and 16-bit samples on the device (vf_png_decode_full):
    an interlaced file gives the pixels of the same image stored plain; the uint8 result of a 16-bit sample is its high
    byte (libpng's png_set_strip_16, Pillow's result), and dtype "float" of a 16-bit file is sample / 65535 on the whole
    sample, written with every other file's byte / 255 by the expansion kernel itself.  Plain and interlaced, 8-bit and
    16-bit items may be mixed; the results come back in item order as views of one buffer.  What still goes to the
    fallback or raises with its reason: a colour file with channels=1, tRNS on a grey or RGB file with channels=None, a
    side above 16384, IDAT data above 256 MiB, an inflated size of 2^31 bytes or more.  The default leaves every result
    and every error as it was."""
    assert channels in (None, 1, 3), "channels is None (the file's own), 1 or 3"
    assert dtype in ("uint8", "float"), "dtype is 'uint8' or 'float'"
    B = get_backend()

    def refuse(info, ch):
        if ch == 1 and info["color_type"] in (2, 3, 6):
            return "colour file with channels=1"
        if ch is None and info["trns_entries"] and info["color_type"] != 3:
            return "tRNS on colour type %d with the file's channels" % info["color_type"]

    shape_of = lambda info: (info["height"], info["width"], channels or info["channels"])
    if full:
        kind = 1 if dtype == "float" else 0
        out = _decode_files("decode_png", [_file_bytes(it) for it in items], channels, fallback,
                            lambda f: png_inspect_full(f, passes=False), refuse,
                            lambda files, infos: B.png_decode_full(files, channels, infos, kind), PNG_STATUS,
                            "corrupt image data", shape_of, stack and not kind)
        if kind:   # what the fallback gave is bytes
            out = [B.png_bytes_to_float(t) if t.dtype == torch.uint8 else t for t in out]
            out = _stacked(out, None, []) if stack else out
        return out
    out = _decode_files("decode_png", [_file_bytes(it) for it in items], channels, fallback, png_inspect, refuse,
                        lambda files, infos: B.png_decode(files, channels, infos), PNG_STATUS, "corrupt image data",
                        shape_of, stack)
    return _as_float(B, out) if dtype == "float" else out


def _as_float(B, out):
    """dtype="float" of the PNG decoders: b / 255 of one tensor or of each of a list."""
    return B.png_bytes_to_float(out) if torch.is_tensor(out) else [B.png_bytes_to_float(t) for t in out]


def decode_image(items, channels=3, stack=False, fallback=None, dtype="uint8", progressive=False, full=False, layouts=False):
    """image.load(path, channels) for a mixed folder: every item's signature says whether it is a JPEG or a PNG file; the
    JPEGs go to decode_jpeg and the PNGs to decode_png, one call each, and the results come back in the caller's order.
    progressive is decode_jpeg's: True decodes progressive JPEG files on the device as well.  full is decode_png's: True
    decodes Adam7-interlaced and 16-bit PNG files on the device as well (a 16-bit sample gives its high byte; dtype
    "float" divides those bytes by 255 here, as it does for the JPEGs).  layouts is decode_jpeg's too: True decodes the
    other samplings, RGB files and sequential files of several scans on the device (and implies progressive).  ValueError
    naming the item for a file that is neither."""
    B = get_backend()
    files = [_file_bytes(it) for it in items]
    jpg, png = [], []
    for i, f in enumerate(files):
        if f[:2] == b"\xff\xd8":
            jpg.append(i)
        elif f[:8] == b"\x89PNG\r\n\x1a\n":
            png.append(i)
        else:
            raise ValueError("decode_image: item %d is neither a JPEG nor a PNG file" % i)
    out = [None] * len(files)
    for idx, dec, name, more in ((jpg, decode_jpeg, "decode_jpeg",
                                  {"layouts": True} if layouts else {"progressive": True} if progressive else {}),
                                 (png, decode_png, "decode_png", {"full": True} if full else {})):
        if not idx:
            continue
        try:
            got = dec([files[i] for i in idx], channels=channels, fallback=fallback, **more)
        except ValueError as e:   # the item's number in the caller's list
            m = re.match(r"%s: item (\d+)(.*)" % name, str(e), re.S)
            if m is None:
                raise
            raise ValueError("%s: item %d%s" % (name, idx[int(m.group(1))], m.group(2))) from None
        for i, t in zip(idx, got):
            out[i] = t
    if stack:
        out = _stacked(out, None, [])
    return _as_float(B, out) if dtype == "float" else out


def load_mask(item, full=False):
    """`image.load(maskName):byte()` of datavid/donkey_folder.lua for a PNG mask: the file's own channels decoded on the
    device, then byte_mask (only 255 becomes 1).  uint8 H x W (a grey file) or H x W x C on the device, ready for
    ClipBatcher.set_mask, PatchArrayBatcher.set_mask and inference.load_whole_frames.  full=True takes an
    Adam7-interlaced or 16-bit mask too (decode_png's full=True; of a 16-bit sample the high byte is compared with 255)."""
    (m,) = decode_png([item], full=full)
    m = byte_mask(m)
    return m[..., 0].contiguous() if m.shape[2] == 1 else m


def _files_from(buf, offsets):
    """The files of an encoder's (device buffer, device offsets) as a list of `bytes`: one offsets read, which synchronises,
    and one device-to-host copy of the bytes in use (the files end at offsets[-1])."""
    offs = offsets.cpu().tolist()
    host = buf[:offs[-1]].cpu().numpy().tobytes()
    return [host[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def _as_frames(who, frames, ndim):
    """An encoder's input as a tensor of `ndim` dimensions: uint8 as it is, any float as float32.  ValueError naming the
    encoder for another rank or dtype."""
    t = torch.as_tensor(frames)
    if t.dim() != ndim:
        raise ValueError("%s: frames of %d dimensions; a batch is %s" % (who, t.dim(), {
            4: "uint8 N x H x W x C or float N x C x H x W",
            5: "uint8 G x N x H x W x 3 or float G x N x 3 x H x W (4-D: one clip)"}[ndim]))
    if t.dtype != torch.uint8:
        if not t.is_floating_point():
            raise ValueError("%s: frames of dtype %s; they are uint8 or float" % (who, t.dtype))
        t = t.float()
    return t


# ------------------------------------------------------------------------------------------------- PNG
def encode_png(frames, level=0):
    """image.save of a batch of frames as PNG, encoded on the device in one call (vf_png_encode): a list of `bytes`, one
    whole PNG file per frame.  frames: uint8 N x H x W x C (stored as they are) or float N x C x H x W (image.savePNG's
    rule: saturated to [0,1], times 255 in float32, truncated); C = 1 (grey) or 3 (RGB); host or device.  Decoding a
    file gives exactly those bytes; the file bytes depend on the frame alone and are the same on every run.  level: 0, the
    fast encoder, or 1, "dense" (vf_png_encode_level): chained matches over the chunk and the 8 KiB of the
    frame's stream before it, about half the bytes on smooth frames for a slower deflate stage; anything else is a
    ValueError naming `level`.  One device-to-host copy brings the batch back."""
    from .backend import png_level
    level = png_level("encode_png", level)
    t = _as_frames("encode_png", frames, 4)
    B = get_backend()
    return _files_from(*B.png_encode(B.from_host(t).contiguous(), level))


# ------------------------------------------------------------------------------------------------ JPEG
def _jpeg_options(who, restart_rows, restart_blocks, optimize, progressive=False):
    """The encoder's options as (rows, blocks, optimize, progressive) of ints; ValueError naming the argument for a bad value,
    and for a restart interval asked of a progressive file."""
    import numbers
    if not isinstance(progressive, (bool, np.bool_)):
        raise ValueError("%s: progressive=%r is not True or False" % (who, progressive))
    for name, v in (("restart_rows", restart_rows), ("restart_blocks", restart_blocks)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= 65535:
            raise ValueError("%s: %s=%r is not an integer from 0 to 65535" % (who, name, v))
    if not isinstance(optimize, (bool, np.bool_)):
        raise ValueError("%s: optimize=%r is not True or False" % (who, optimize))
    for name, v in (("restart_rows", restart_rows), ("restart_blocks", restart_blocks)):
        if progressive and v:
            raise ValueError("%s: %s=%r with progressive=True (a progressive file has no restart intervals here)" % (who, name, v))
    return int(restart_rows), int(restart_blocks), int(optimize), int(progressive)


def encode_jpeg(frames, quality=75, subsampling="420", restart_rows=0, restart_blocks=0, optimize=False, progressive=False):
    """image.save('x.jpg') / image.compressJPG of a batch of frames, encoded on the device in one call (vf_jpeg_encode): a
    list of `bytes`, one whole baseline JFIF file per frame, byte for byte what libjpeg's default compression — Pillow's
    save(format="JPEG", quality=quality, subsampling=...) — writes.  frames: uint8 N x H x W x C (taken as they are) or
    float N x C x H x W (image.savePNG's rule, which is saveJPG's too: saturated to [0,1], times 255 in float32,
    truncated); C = 1 (grey) or 3 (RGB, coded as YCbCr); host or device.  quality: 1 to 100.  subsampling: "420" (the
    default of libjpeg and Pillow), "422" or "444"; grey frames ignore it.  restart_rows, restart_blocks, optimize: Pillow's
    restart_marker_rows, restart_marker_blocks and optimize, with the same bytes: a restart interval of so many rows of
    MCUs or of so many MCUs (0 to 65535 each; rows win, clamped to 65535 MCUs), which decode_jpeg decodes a segment per
    workgroup, and Huffman tables made from each file's own symbol counts (smaller files; the header differs from file to
    file).  progressive: Pillow's progressive=True with the same bytes (vf_jpeg_encode_prog): SOF2, libjpeg's 10 scans (grey:
    6), each behind its own optimal tables; optimize changes nothing then, as in libjpeg, and a non-zero restart_rows or
    restart_blocks with it is a ValueError.  The defaults write the default file.  The files are what decode_jpeg reads.  A bad quality, subsampling,
    option, rank or dtype is a ValueError naming the argument.  One device-to-host copy brings the batch back."""
    import numbers
    from .backend import JPEG_SUBSAMPLING
    if isinstance(quality, bool) or not isinstance(quality, numbers.Integral) or not 1 <= quality <= 100:
        raise ValueError("encode_jpeg: quality=%r is not an integer from 1 to 100" % (quality,))
    if subsampling not in JPEG_SUBSAMPLING:
        raise ValueError("encode_jpeg: subsampling=%r is not one of %s" % (subsampling, ", ".join(map(repr, sorted(JPEG_SUBSAMPLING)))))
    opts = _jpeg_options("encode_jpeg", restart_rows, restart_blocks, optimize, progressive)
    t = _as_frames("encode_jpeg", frames, 4)
    B = get_backend()
    return _files_from(*B.jpeg_encode(B.from_host(t).contiguous(), int(quality), subsampling, *opts))


# ------------------------------------------------------------------------------------------------- GIF
def encode_gif(clips, delay=10):
    """`convert -delay D frame_1.png ... clip.gif` of a batch of clips, encoded on the device in one call
    (vf_gif_encode): a list of `bytes`, one whole animated GIF89a file per clip, looping forever, `delay` centiseconds a
    frame.  clips: uint8 G x N x H x W x 3 (taken as they are) or float G x N x 3 x H x W (image.savePNG's rule, the
    bytes `convert` would read from the PNGs); a 4-D input is one clip; host or device; RGB only.  Every frame carries
    its own table of 256 colours: its own colours when it has at most 256 (lossless), else a median cut; no dithering
    (DESIGN 5.5 has the rule, which is this project's own, not ImageMagick's).  A file's bytes depend on its frames and
    the delay alone and are the same on every run.  One device-to-host copy brings the batch back."""
    t = torch.as_tensor(clips)
    t = _as_frames("encode_gif", t.unsqueeze(0) if t.dim() == 4 else t, 5)
    if int(delay) != delay or not 0 <= delay <= 65535:
        raise ValueError("encode_gif: delay=%r is not a whole number of centiseconds from 0 to 65535" % (delay,))
    B = get_backend()
    return _files_from(*B.gif_encode(B.from_host(t).contiguous(), int(delay)))


# ------------------------------------------------------------------------------------------------ APNG
def encode_apng(clips, delay=10, loop=0, level=0):
    """A batch of clips as animated PNG files, lossless, encoded on the device in one call (vf_apng_encode): a list of
    `bytes`, one whole APNG file per clip, `delay` centiseconds a frame, played `loop` times (0: forever).  clips: uint8
    G x N x H x W x C (taken as they are) or float G x N x C x H x W (image.savePNG's rule); C = 1 (grey) or 3 (RGB); a
    4-D input is one clip; host or device.  The file is what tests/apng_ref.py assembles from the N files encode_png
    writes for the clip's frames: every frame is its own zlib stream, frame 0 in IDAT chunks — the file is
    also a PNG of frame 0 — and the others in fdAT chunks; no frame differencing.  Decoding gives exactly the frames'
    bytes; a file's bytes depend on its frames, delay and loop alone and are the same on every run.  level is
    encode_png's: the file is assembled from the frames' files of that level.  One device-to-host copy brings the batch
    back."""
    from .backend import png_level
    level = png_level("encode_apng", level)
    t = torch.as_tensor(clips)
    t = _as_frames("encode_apng", t.unsqueeze(0) if t.dim() == 4 else t, 5)
    if int(delay) != delay or not 0 <= delay <= 65535:
        raise ValueError("encode_apng: delay=%r is not a whole number of centiseconds from 0 to 65535" % (delay,))
    if int(loop) != loop or not 0 <= loop <= 65535:
        raise ValueError("encode_apng: loop=%r is not a whole number of plays from 0 to 65535 (0: forever)" % (loop,))
    B = get_backend()
    return _files_from(*B.apng_encode(B.from_host(t).contiguous(), int(delay), int(loop), level))


def apng_info(item):
    """The host-side walk of one APNG or PNG file (no GPU): dict(width, height, bit_depth, color_type, interlace, channels
    (of the decoded frames), frames, num_plays (-1 without acTL; 0: forever), supported, animated, default_is_frame,
    palette_entries, reason, frame_info), frame_info holding per frame dict(x, y, w, h, delay_num, delay_den, dispose,
    blend, data_bytes).  A PNG without acTL is a clip of one frame.  ValueError if the file is malformed (DESIGN 5.11
    lists what that is: CRCs, acTL, sequence numbers, frames without data or outside the canvas, truncation)."""
    return apng_inspect(_file_bytes(item))


def decode_apng(items, alpha=False, fallback=None):
    """The frames of a batch of APNG files, decoded and composited on the device (vf_apng_decode): a list with one device
    uint8 N x H x W x 3 tensor per file (N x H x W x 4 with alpha=True), views of one buffer.  Output frame k is the
    canvas after frame k was rendered, by the APNG specification (tests/apng_decode_ref.py is the
    definition): the canvas starts transparent black, blend SOURCE replaces the frame's rectangle, dispose 1 clears it, 2
    restores what was there; grey is replicated, a file without alpha paints alpha 255, a pixel nothing has painted is
    (0,0,0) with alpha 0; a 16-bit sample gives its high byte.  Every format decode_png(full=True) takes works, Adam7
    too.  A PNG without acTL is a clip of one frame.  Files `encode_apng` wrote come back as their frames' exact bytes.

    items: bytes, uint8 arrays or paths.  Files the device decoder does not take (blend OVER with alpha, tRNS on grey or
    RGB, a side above 16384, more than 65535 frames, 2 GiB of frames) go to fallback(bytes), which returns the uint8
    N x H x W x C frames; without it they raise ValueError naming the item and why.  A malformed file raises ValueError
    naming the item before anything is launched; a corrupt frame stream raises it, with the status, once the stream has
    synchronised.  A batch of more than 65535 frames is decoded in several calls."""
    from .backend import APNG_MAX_BATCH_FRAMES
    B = get_backend()
    oc = 4 if alpha else 3
    files = [_file_bytes(it) for it in items]
    infos, dev, out = {}, [], [None] * len(files)
    for i, f in enumerate(files):
        try:
            info = apng_inspect(f)
        except ValueError as e:
            raise ValueError("decode_apng: item %d: %s" % (i, e)) from None
        if not info["supported"]:
            if fallback is None:
                raise ValueError("decode_apng: item %d is not supported by the device decoder: %s" % (i, info["reason"]))
            fr = torch.as_tensor(np.ascontiguousarray(fallback(f)))
            assert fr.dtype == torch.uint8 and fr.dim() == 4 and fr.shape[3] == oc, \
                "fallback returns uint8 N x H x W x %d, got %s %s" % (oc, fr.dtype, tuple(fr.shape))
            out[i] = B.from_host(fr).contiguous()
            continue
        infos[i] = info
        dev.append(i)
    calls, count = [[]], 0
    for i in dev:                                        # a call holds 65535 frames at most
        if calls[-1] and count + infos[i]["frames"] > APNG_MAX_BATCH_FRAMES:
            calls.append([])
            count = 0
        calls[-1].append(i)
        count += infos[i]["frames"]
    results = []
    for part in calls:
        if not part:
            continue
        try:
            results.append((part, B.apng_decode([files[i] for i in part], alpha, [infos[i] for i in part])))
        except VfError as e:   # found on the host while the batch was planned: nothing was launched
            m = re.search(r"image (\d+)", str(e))
            if m is None:
                raise
            raise ValueError("decode_apng: item %d: %s" % (part[int(m.group(1))], e)) from None
    for part, (buf, offs, status) in results:
        st = status.cpu().tolist()
        for j, i in enumerate(part):
            if st[j] != 0:
                raise ValueError("decode_apng: item %d: corrupt image data (%s)" % (i, PNG_STATUS.get(st[j], st[j])))
            s = infos[i]
            out[i] = buf[offs[j]:offs[j + 1]].view(s["frames"], s["height"], s["width"], oc)
    return out


# ------------------------------------------------------------------------------------------ GIF decode
def gif_info(item):
    """The host-side walk of one GIF87a / GIF89a file (no GPU): dict(width, height, frames, loop (-1 without a NETSCAPE2.0
    block), supported, global_table_size, version, rect_pixels, reason, frame_info), frame_info holding per frame
    dict(delay, disposal, x, y, w, h, interlace, transparency (index or -1), table_size, local_table, min_code_size,
    data_bytes).  ValueError if the file is malformed (signature, truncation, no trailer, a rectangle that leaves the
    screen, a frame without a colour table, a minimum code size outside 2 .. 8)."""
    return gif_inspect(_file_bytes(item))


def decode_gif(items, alpha=False, fallback=None):
    """The frames of a batch of GIF files, decoded and composited on the device in one call (vf_gif_decode): a list with
    one device uint8 N x H x W x 3 tensor per file (N x H x W x 4 with alpha=True), views of one buffer.  Output frame k
    is the canvas after frame k was painted, by the browsers' rule (tests/gif_decode_ref.py is the
    definition): the canvas starts transparent, disposal 2 clears the frame's rectangle, 3 restores what was there; a
    pixel nothing has painted is (0,0,0) and, with alpha, has alpha 0.  Files `encode_gif` wrote come back as their
    quantised frames.

    items: bytes, uint8 arrays or paths.  Files the device decoder does not take (a side above 16384, more than 65535
    frames, 2 GiB of frames) go to fallback(bytes), which returns the uint8 N x H x W x C frames; without it they raise
    ValueError naming the item and why.  A malformed file raises ValueError naming the item before anything is launched;
    a corrupt code stream or a colour index beyond its table raises it, with the status, once the stream has
    synchronised."""
    B = get_backend()
    oc = 4 if alpha else 3
    files = [_file_bytes(it) for it in items]
    infos, dev, out = [], [], [None] * len(files)
    for i, f in enumerate(files):
        try:
            info = gif_inspect(f)
        except ValueError as e:
            raise ValueError("decode_gif: item %d: %s" % (i, e)) from None
        if not info["supported"]:
            if fallback is None:
                raise ValueError("decode_gif: item %d is not supported by the device decoder: %s" % (i, info["reason"]))
            fr = torch.as_tensor(np.ascontiguousarray(fallback(f)))
            assert fr.dtype == torch.uint8 and fr.dim() == 4 and fr.shape[3] == oc, \
                "fallback returns uint8 N x H x W x %d, got %s %s" % (oc, fr.dtype, tuple(fr.shape))
            out[i] = B.from_host(fr).contiguous()
            continue
        infos.append(info)
        dev.append(i)
    if dev:
        try:
            buf, offs, status = B.gif_decode([files[i] for i in dev], alpha, infos)
        except VfError as e:   # found on the host while the batch was planned: nothing was launched
            m = re.search(r"image (\d+)", str(e))
            if m is None:
                raise
            raise ValueError("decode_gif: item %d: %s" % (dev[int(m.group(1))], e)) from None
        st = status.cpu().tolist()
        for j, i in enumerate(dev):
            if st[j] != 0:
                raise ValueError("decode_gif: item %d: corrupt image data (%s)" % (i, GIF_STATUS.get(st[j], st[j])))
            s = infos[j]
            out[i] = buf[offs[j]:offs[j + 1]].view(s["frames"], s["height"], s["width"], oc)
    return out


# --------------------------------------------------------------------------------------------- scores
def _check_metric_args(a, b, mask, valid):
    """frame_metrics' argument checks, on the host and before any backend exists: -> (a, b, mask, (vh, vw)) as tensors,
    floats as float32."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    same_kind = (a.dtype == torch.uint8) == (b.dtype == torch.uint8) and (a.dtype == torch.uint8 or (a.is_floating_point() and b.is_floating_point()))
    if a.dim() != 4 or tuple(a.shape) != tuple(b.shape) or not same_kind:
        raise ValueError("frame_metrics: a is %s %s and b is %s %s; both are float N x C x H x W or both uint8 N x H x W x C"
                         % (str(a.dtype).replace("torch.", ""), tuple(a.shape), str(b.dtype).replace("torch.", ""), tuple(b.shape)))
    if a.dtype == torch.uint8:
        n, H, W, Cc = a.shape
    else:
        a, b = a.float(), b.float()
        n, Cc, H, W = a.shape
    if Cc not in (1, 3):
        raise ValueError("frame_metrics: %d channels; frames have 1 (grey) or 3 (RGB)" % Cc)
    if n < 1 or H < 1 or W < 1:
        raise ValueError("frame_metrics: an empty batch of shape %s" % (tuple(a.shape),))
    if mask is not None:
        mask = torch.as_tensor(mask)
        if mask.dtype == torch.bool:
            mask = mask.to(torch.uint8)
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (H, W):
            raise ValueError("frame_metrics: the mask is %s %s; it is uint8 H x W = %d x %d, non-zero = hole"
                             % (str(mask.dtype).replace("torch.", ""), tuple(mask.shape), H, W))
    vh, vw = (H, W) if valid is None else valid
    if int(vh) != vh or int(vw) != vw or not (1 <= vh <= H and 1 <= vw <= W):
        raise ValueError("frame_metrics: valid=%r is outside 1..%d x 1..%d (rows, columns of the frame that count)" % (valid, H, W))
    return a, b, mask, (int(vh), int(vw))


def frame_metrics(a, b, mask=None, valid=None, clip=True):
    """The scores of the result frames a against the truth b, computed where the frames are, in one call
    (vf_frame_metrics): -> (table, METRIC_COLUMNS), table a device int64 tensor N x 2 x 6 — per frame and region (0: every
    valid pixel; 1: the valid pixels under the mask, all zero without one), summed over the channels, the integer sums
    n, sse, sae, ssim_q, ssim_n, flicker of DESIGN.md 5.7.  a, b: both float N x C x H x W in [0,1] (image.savePNG's rule
    makes the bytes save_frames would write) or both uint8 N x H x W x C; C = 1 or 3; host or device.  mask: uint8 H x W,
    non-zero = hole.  valid = (vh, vw): only rows < vh and columns < vw count; the rest (the bottom-right padding of the
    whole-frame driver) is never read.  clip: the batch is one clip, and flicker — sum |(a_t - a_{t-1}) - (b_t - b_{t-1})|
    for t >= 1 — runs over it; False: independent images, flicker 0.  Every column is an integer sum: the table equals
    tests/metrics_ref.py exactly and is the same on every run.  ValueError, naming the argument, before anything is
    launched, for a and b of different shapes or types, C outside {1, 3}, a mask of another shape, valid outside the frame.
    inference.evaluate_frames turns the table into PSNR, SSIM, mean absolute error and flicker."""
    a, b, mask, valid = _check_metric_args(a, b, mask, valid)
    B = get_backend()
    m = None if mask is None else B.from_host(mask).contiguous()
    return B.frame_metrics(B.from_host(a).contiguous(), B.from_host(b).contiguous(), m, valid, clip), METRIC_COLUMNS


# ---------------------------------------------------------------------------------------------- image.scale
def load_size(H, W, loadSize, scalef=None):
    """(height, width) that loadImage / loadContImages (data/donkey_folder.lua:40-62, datavid/donkey_folder.lua:84-102)
    scale an H x W image to.  loadSize > 0: the shorter side becomes loadSize, the other keeps the aspect ratio
    (Lua arithmetic in double, truncated by the tensor constructor).  loadSize < 0: `image.scale(input, iH, iW)` with
    iH = scalef*H, iW = scalef*W — the reference passes the scaled HEIGHT as the width, so the aspect is transposed;
    kept.  loadSize == 0: unchanged."""
    if loadSize > 0:
        if W < H:
            return int(loadSize * H / W), int(loadSize)   # image.scale(input, loadSize, loadSize * iH / iW)
        return int(loadSize), int(loadSize * W / H)       # image.scale(input, loadSize * iW / iH, loadSize)
    if loadSize < 0:
        assert scalef is not None, "loadSize < 0 needs the random scale factor (draw_scalef)"
        return int(scalef * W), int(scalef * H)
    return int(H), int(W)


def draw_scalef(loadSize, rng):
    """The random scale of loadSize < 0: uniform in [0.5, 1.5] for -1, in [1, 3] for any other negative value."""
    return float(rng.uniform(0.5, 1.5)) if loadSize == -1 else float(rng.uniform(1, 3))


def _patch_array_shape(nc, array_h, array_w):
    """the conditions of the patch-array hook that do not depend on a frame"""
    if nc != 3:
        raise ValueError("patch array: nc=%d, the hook writes channel triples (nc must be 3)" % nc)
    if array_h < 2 or array_w < 2:
        raise ValueError("patch array: a %dx%d array needs at least 2 windows a side" % (array_h, array_w))


def patch_array_steps(height, width, fineSize, array_h=3, array_w=3, nc=3, crop_h=1, crop_w=1):
    """(steph, stepw) of the window loop of datavid/donkey_wholeim.lua:153-154,196-197 over a height x width scaled frame,
    or ValueError naming the geometry where the reference is not defined: the hook hard-codes 3 channels; a step below 2
    leaves `out` channels unwritten (floor(h/steph) no longer numbers the rows from 0); a loop that visits more than
    array_h x array_w windows indexes past `masked`; a crop beyond the frame has no source."""
    fs = int(fineSize)
    where = "a %dx%d array of %d-pixel windows over the %dx%d scaled frame" % (array_h, array_w, fs, height, width)
    _patch_array_shape(nc, array_h, array_w)
    steph = (height - fs) // (array_h - 1) if height >= fs else 0
    stepw = (width - fs) // (array_w - 1) if width >= fs else 0
    if steph < 2 or stepw < 2:
        raise ValueError("patch array: %s gives steps %d and %d (both must be >= 2)" % (where, steph, stepw))
    nh, nw = (height - fs) // steph + 1, (width - fs) // stepw + 1
    if (nh, nw) != (array_h, array_w):
        raise ValueError("patch array: %s: steps %d and %d visit %dx%d windows" % (where, steph, stepw, nh, nw))
    if not (1 <= crop_h <= height and 1 <= crop_w <= width):
        raise ValueError("patch array: crop (%d,%d) outside the %dx%d scaled frame" % (crop_w, crop_h, height, width))
    return steph, stepw


def draw_patch_array(H, W, loadSize, rng):
    """The random decisions of train_wholeim_input.lua's loader for an H x W frame, in its order (host only):
    scalef when loadSize < 0 (datavid/donkey_wholeim.lua:61-67), crop_w = torch.random(100), crop_h = torch.random(70)
    (:167-168, 1-based), the flip uniform > 0.6 (:177).  -> {height, width, crop_w, crop_h, flip}."""
    scalef = draw_scalef(loadSize, rng) if loadSize < 0 else None
    height, width = load_size(H, W, loadSize, scalef)
    crop_w = int(rng.integers(1, 101))
    crop_h = int(rng.integers(1, 71))
    flip = bool(rng.uniform() > 0.6)
    return dict(height=height, width=width, crop_w=crop_w, crop_h=crop_h, flip=flip)


def byte_mask(decoded):
    """`image.load(maskName):byte()` of a decoded uint8 mask image: the [0,1] float image truncated to Byte, so only
    255 becomes 1.  Host or device tensor / array in, uint8 tensor (same place) out."""
    m = torch.as_tensor(decoded)
    return (m == 255).to(torch.uint8)


def _frames(x, hwc):
    """(device tensor, N, C, H, W) of one frame or a stack: hwc -> uint8 [N x] H x W x C (a decoder's interleaved
    output; H x W for one channel), else [N x] C x H x W planar."""
    B = get_backend()
    t = torch.as_tensor(x)
    if hwc:
        assert t.dtype == torch.uint8, "decoded frames are uint8 H x W x C"
        if t.dim() == 2:
            t = t.unsqueeze(-1)
        t = t if t.dim() == 4 else t.unsqueeze(0)
        N, H, W, C = t.shape
    else:
        t = t.float() if t.is_floating_point() else t
        t = t if t.dim() == 4 else t.unsqueeze(0)
        N, C, H, W = t.shape
    return B.from_host(t).contiguous(), N, C, H, W


def image_scale(x, width, height, layout="chw"):
    """Torch7 `image.scale(x, width, height)` (bilinear; Torch7 argument order, fractional sizes truncated) on the
    device, bit-identical to image.c's float32 arithmetic.  A leading frame axis resizes N frames in one launch.
      float [N x] C x H x W                 -> float planar [N x] C x height x width (the Float path);
      uint8 [N x] C x H x W                 -> uint8 (the Byte path: masks; intermediate rounded as a ByteTensor);
      uint8 [N x] H x W x C, layout="hwc"   -> decoded frames read as b / 255 (image.load(path, nc, 'float')),
                                               float planar [N x] C x height x width.
    Host or device tensors in; device tensors out."""
    B = get_backend()
    width, height = int(width), int(height)
    t = torch.as_tensor(x)
    single = t.dim() in (2, 3) if layout == "hwc" else t.dim() == 3
    if layout == "hwc":
        src, N, C, H, W = _frames(t, True)
        out = B.empty(N, C, height, width)
        B.image_scale(src, True, out)
    elif t.dtype == torch.uint8:
        src, N, C, H, W = _frames(t, False)
        out = B.empty(N, C, height, width, dtype=torch.uint8)
        B.image_scale_u8(src, out)
    else:
        src, N, C, H, W = _frames(t, False)
        out = B.empty(N, C, height, width)
        B.image_scale(src, False, out)
    return out[0] if single else out


class ImageBatcher:
    """train.lua's loader (data/donkey_folder.lua:40-88: loadImage + trainHook) feeding CenterTrainer.set_batch.

    add(image) takes ONE decoded image (uint8 H x W x nc, or float nc x H x W in [0,1]; host or device), draws the
    loader's random numbers from `rng` in its order (scalef when loadSize < 0, then h1, w1, flip) — they depend only
    on the scaled SIZES — and launches one kernel that resizes, crops, flips and maps to [-1,1] straight into row `n`
    of the B x nc x fineSize x fineSize batch, evaluating only the crop's pixels.  batch() returns that planar batch."""

    def __init__(self, batchSize, nc=3, fineSize=128, loadSize=350, rng=None):
        B = get_backend()
        self.B, self.nc, self.fs, self.loadSize = batchSize, nc, fineSize, loadSize
        self.rng = rng or np.random.default_rng()
        self.out = B.empty(batchSize, nc, fineSize, fineSize)
        self.n = 0

    def draw(self, H, W):
        """The loader's decisions for an H x W image: {height, width, h1, w1, flip} (0-based corner, clamped as in
        ClipBatcher.draw)."""
        fs, rng = self.fs, self.rng
        scalef = draw_scalef(self.loadSize, rng) if self.loadSize < 0 else None
        height, width = load_size(H, W, self.loadSize, scalef)
        assert height >= fs and width >= fs, "the %dx%d scaled image is smaller than fineSize=%d" % (height, width, fs)
        h1 = int(math.ceil(rng.uniform(1e-2, height - fs)))      # :76-77
        w1 = int(math.ceil(rng.uniform(1e-2, width - fs)))
        flip = bool(rng.uniform() > 0.5)                          # :82
        return dict(height=height, width=width, h1=min(h1, height - fs), w1=min(w1, width - fs), flip=flip)

    def add(self, image, decisions=None):
        """Returns the decisions used."""
        B = get_backend()
        assert self.n < self.B, "batch is full"
        t = torch.as_tensor(image)
        hwc = t.dtype == torch.uint8
        src, N, C, H, W = _frames(t, hwc)
        assert N == 1 and C == self.nc, "one %d-channel image, got %d x %d channels" % (self.nc, N, C)
        d = decisions if decisions is not None else self.draw(H, W)
        B.image_hook2d(src, hwc, self.out[self.n], d["height"], d["width"], d["w1"], d["h1"], d["flip"])
        self.n += 1
        return d

    def batch(self):
        """B x nc x fineSize x fineSize planar in [-1,1] on the device (the loader's batch of train.lua:282)."""
        assert self.n == self.B, "batch holds %d of %d samples" % (self.n, self.B)
        self.n = 0
        return self.out


def center_prepare(batch, overlapPred, fill=CENTER_FILL, out=None):
    """train.lua:284-298: (input_ctx, real_center) as channels-last device tensors from the loader's batch
    (B x nc x fs x fs in [-1,1], host or device).  out = (input_ctx, real_center): write into these existing tensors
    (a captured HIP graph keeps reading the buffers it was captured with)."""
    B = get_backend()
    x = B.from_host(batch).float().contiguous()
    nB, nc, fs, _ = x.shape
    dev = x.device
    fillv = [2 * m / 255.0 - 1.0 for m in fill]
    fillv = (fillv * ((nc + len(fillv) - 1) // len(fillv)))[:nc]
    if out is not None and tuple(out[0].shape) == (nB, nc, fs, fs) and tuple(out[1].shape) == (nB, nc, fs // 2, fs // 2):
        ctx, center = out
    else:
        ctx = nhwc_empty(nB, nc, fs, fs, dev)
        center = nhwc_empty(nB, nc, fs // 2, fs // 2, dev)
    B.center_prepare(x, ctx, center, B.from_host(torch.tensor(fillv, dtype=torch.float32)), overlapPred)
    return ctx, center


class ClipBatcher:
    """trainHook of datavid/donkey_folder.lua:135-189 feeding the (ctx, full, mask) batch of datavid/dataset.lua:426.

    add(clip, mask) takes ONE decoded, scaled clip ((predLen*nc) x iH x iW float in [0,1], host numpy) and the scaled
    Byte mask (1 x iH x iW), draws the hook's random numbers from `rng` in the hook's order (crop corner, dark-crop
    rejection, random blocks, flip) and, unless the sample is rejected, launches one kernel that writes row `n` of the
    three batch tensors.  batch() returns them (channels-last, on the device) for VidTrainer.set_batch."""

    def __init__(self, batchSize, channels, fineSize=128, maskValue=110.0 / 255.0, rng=None):
        B = get_backend()
        self.B, self.C, self.fs, self.maskValue = batchSize, channels, fineSize, float(maskValue)
        self.rng = rng or np.random.default_rng()
        dev = B.device
        self.full = nhwc_empty(batchSize, channels, fineSize, fineSize, dev)
        self.masked = nhwc_empty(batchSize, channels, fineSize, fineSize, dev)
        self.mask = nhwc_empty(batchSize, channels, fineSize, fineSize, dev)
        self.n = 0

    def draw(self, clip, mask):
        """The hook's decisions for one sample (host side, no pixels touched beyond two reductions)."""
        fs = self.fs
        _, iH, iW = clip.shape
        return self._decide(iH, iW, lambda h1, w1: (float(clip[:, h1:h1 + fs, w1:w1 + fs].mean()),
                                                    mask[:, h1:h1 + fs, w1:w1 + fs].max()))

    def _decide(self, iH, iW, crop_stats):
        """The hook's draws in its order; crop_stats(h1, w1) -> (mean of the clip's crop, max of the mask's crop)."""
        fs, rng = self.fs, self.rng
        h1 = int(math.ceil(rng.uniform(1e-2, iH - fs)))          # :145-146 (1-based corner; image.crop takes it 0-based)
        w1 = int(math.ceil(rng.uniform(1e-2, iW - fs)))
        h1, w1 = min(h1, iH - fs), min(w1, iW - fs)
        crop_mean, mask_max = crop_stats(h1, w1)
        if crop_mean < 0.1 and rng.uniform() > 0.05:              # :148-153: dark crops are mostly rejected
            return None
        blocks, bs = None, fs // 6
        if not (mask_max > 0.5):                                  # :165-169
            nBlocks = int(rng.integers(2, 11))                   # torch.random(2, maxBlocks)
            blocks = [(int(rng.integers(3, fs - bs - 1)), int(rng.integers(3, fs - bs - 1))) for _ in range(nBlocks)]
        flip = bool(rng.uniform() > 0.5)                          # :178
        return dict(w1=w1, h1=h1, flip=flip, blocks=blocks, blockSize=bs)

    def set_mask(self, mask):
        """The loader's module-global Byte mask (datavid/donkey_folder.lua:33-35; `byte_mask` makes it from a decoded
        image): 0/1 uint8 [1 x] H x W.  add_frames rescales it in place of the old one on every call."""
        m = torch.as_tensor(mask)
        assert m.dtype == torch.uint8, "the mask is a ByteTensor (byte_mask)"
        self.mask_state = get_backend().from_host(m.reshape(1, m.shape[-2], m.shape[-1])).contiguous()

    mask_state = last = None

    def add_frames(self, frames, loadSize=0, decisions=None):
        """loadContImages + trainHook (datavid/donkey_folder.lua:71-189) on the device for ONE clip of decoded frames
        (uint8 predLen x H x W x nc, or float predLen x nc x H x W in [0,1]; host or device).

        Draws scalef (loadSize < 0), scales the channel-stacked clip (image.scale), and — as the reference does on
        every call, rejected samples included — replaces the mask state by `image.scale(mask, W, H)` of the PREVIOUS
        state on the Byte path (with loadSize < 0 it degrades from call to call, as in the reference).  Then the hook's
        draws in its order, the dark-crop mean and the mask test read as one device pair (vf_crop_stats, summed in
        double as TH's mean), and the clip_prepare launch of `add`.  Returns True unless the sample is rejected;
        `last` holds the sizes and decisions (None if rejected)."""
        B = get_backend()
        assert self.n < self.B, "batch is full"
        assert self.mask_state is not None, "set_mask() first: the video loader's mask is part of its state"
        t = torch.as_tensor(frames)
        hwc = t.dtype == torch.uint8
        src, N, C, H, W = _frames(t, hwc)
        assert N * C == self.C, "%d frames x %d channels do not make the batcher's %d channels" % (N, C, self.C)
        scalef = None
        if decisions is None and loadSize < 0:
            scalef = draw_scalef(loadSize, self.rng)
        if decisions is not None:
            height, width = decisions["height"], decisions["width"]
        else:
            height, width = load_size(H, W, loadSize, scalef)
        clip = B.empty(N * C, height, width)
        B.image_scale(src, hwc, clip.view(N, C, height, width))
        mask = B.empty(1, height, width, dtype=torch.uint8)
        B.image_scale_u8(self.mask_state.unsqueeze(0), mask.unsqueeze(0))
        self.mask_state = mask
        fs = self.fs
        if decisions is None:
            assert height >= fs and width >= fs, "the %dx%d scaled clip is smaller than fineSize=%d" % (height, width, fs)

            def crop_stats(h1, w1):
                st = B.empty(2, dtype=torch.float64)
                B.crop_stats(clip, mask[0], fs, w1, h1, st)
                s, m = st.tolist()
                return s / (C * N * fs * fs), m

            d = self._decide(height, width, crop_stats)
        else:
            d = decisions
        self.last = None if d is None else dict(d, height=height, width=width)
        if d is None:
            return False
        mask_f = mask[0].float() if d["blocks"] is None else None
        n = self.n
        B.clip_prepare(clip, mask_f, self.full[n:n + 1], self.masked[n:n + 1], self.mask[n:n + 1], d["w1"], d["h1"],
                       d["flip"], self.maskValue, d["blocks"], d["blockSize"])
        self.n += 1
        return True

    def add(self, clip, mask, decisions=None):
        B = get_backend()
        assert self.n < self.B, "batch is full"
        d = decisions if decisions is not None else self.draw(clip, mask)
        if d is None:
            return False
        clip_d = B.from_host(torch.from_numpy(np.ascontiguousarray(clip, np.float32)))
        mask_d = B.from_host(torch.from_numpy(np.ascontiguousarray(mask[0], np.float32))) if d["blocks"] is None else None
        n = self.n
        B.clip_prepare(clip_d, mask_d, self.full[n:n + 1], self.masked[n:n + 1], self.mask[n:n + 1], d["w1"], d["h1"],
                       d["flip"], self.maskValue, d["blocks"], d["blockSize"])
        self.n += 1
        return True

    def batch(self):
        """(real_ctx, real_full, real_mask) — the loader contract of datavid/dataset.lua:426."""
        assert self.n == self.B, "batch holds %d of %d samples" % (self.n, self.B)
        self.n = 0
        return self.masked, self.full, self.mask


class PatchArrayBatcher:
    """train_wholeim_input.lua's loader (datavid/donkey_wholeim.lua:49-74 loadImage, :141-215 trainHook) feeding the
    (ctx, full, mask) batch of datavid/dataset_wholeim.lua:400-429 to VidTrainer(nc_in=3*array_h*array_w, nc_out=12).

    set_mask(mask) takes the loader's module-global Byte mask (`byte_mask`).  add(image) takes ONE decoded frame (uint8
    H x W x 3, or float 3 x H x W in [0,1]; host or device — a view returned by `decode_jpeg` too), rescales the mask
    state from its previous state (on EVERY call, rejected samples included), draws the loader's random numbers from
    `rng` in its order (`draw_patch_array`) and launches one kernel that resizes, fills, shifts, flips and cuts the
    array_h x array_w windows straight into row `n` of the three channels-last batch tensors; the dark test reads the
    top-left window's sum back (double, fixed order) and draws its extra uniform only for a dark sample.  A rejected
    sample does not advance the row: the next one overwrites it.  batch() returns (masked, full, mask)."""

    mask_state = last = None

    def __init__(self, batchSize, nc=3, fineSize=128, loadSize=360, array_h=3, array_w=3, maskValue=110.0 / 255.0, rng=None):
        B = get_backend()
        _patch_array_shape(nc, array_h, array_w)
        self.B, self.nc, self.fs, self.loadSize = batchSize, nc, fineSize, loadSize
        self.arr_h, self.arr_w, self.maskValue = array_h, array_w, float(maskValue)
        self.rng = rng or np.random.default_rng()
        dev = B.device
        self.masked = nhwc_empty(batchSize, nc * array_h * array_w, fineSize, fineSize, dev)
        self.full = nhwc_empty(batchSize, nc * 4, fineSize, fineSize, dev)
        self.mask = nhwc_empty(batchSize, nc * 4, fineSize, fineSize, dev)
        self.total = B.empty(1, dtype=torch.float64)
        self.n = 0

    def set_mask(self, mask):
        """0/1 uint8 [1 x] H x W; add rescales it in place of the old one on every call (datavid/donkey_wholeim.lua:72)."""
        m = torch.as_tensor(mask)
        assert m.dtype == torch.uint8, "the mask is a ByteTensor (byte_mask)"
        self.mask_state = get_backend().from_host(m.reshape(1, m.shape[-2], m.shape[-1])).contiguous()

    def add(self, image, decisions=None):
        """decisions: {height, width, crop_w, crop_h, flip} instead of the draws (the dark rule still draws from `rng`).
        Returns True unless the sample is rejected; `last` holds the sizes and decisions, `mean` and `rejected`."""
        B = get_backend()
        assert self.n < self.B, "batch is full"
        assert self.mask_state is not None, "set_mask() first: the loader's mask is part of its state"
        t = torch.as_tensor(image)
        hwc = t.dtype == torch.uint8
        src, N, C, H, W = _frames(t, hwc)
        assert N == 1 and C == self.nc, "one %d-channel frame, got %d x %d channels" % (self.nc, N, C)
        d = dict(decisions) if decisions is not None else draw_patch_array(H, W, self.loadSize, self.rng)
        height, width = d["height"], d["width"]
        patch_array_steps(height, width, self.fs, self.arr_h, self.arr_w, self.nc, d["crop_h"], d["crop_w"])
        mask = B.empty(1, height, width, dtype=torch.uint8)
        B.image_scale_u8(self.mask_state.unsqueeze(0), mask.unsqueeze(0))          # :72, before the hook, on every call
        self.mask_state = mask
        n = self.n
        B.patch_array_prepare(src, hwc, mask[0], self.masked[n:n + 1], self.full[n:n + 1], self.mask[n:n + 1], self.total,
                              height, width, self.arr_h, self.arr_w, d["crop_w"], d["crop_h"], d["flip"], self.maskValue)
        mean = self.total.item() / (self.nc * self.fs * self.fs)              # :188-189, TH's mean: a double sum / n
        rejected = bool(mean < 0.1 and self.rng.uniform() > 0.1)              # :189-193
        self.last = dict(d, mean=mean, rejected=rejected)
        if not rejected:
            self.n += 1
        return not rejected

    def batch(self):
        """(real_ctx, real_full, real_mask) as train_wholeim_input.lua:394 reads them."""
        assert self.n == self.B, "batch holds %d of %d samples" % (self.n, self.B)
        self.n = 0
        return self.masked, self.full, self.mask
