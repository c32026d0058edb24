"""The case list of tests/test_gpu_routes.py, shared with scripts/ab_conv_outputs.py (its `pass_routes` section and its
`record-routes` mode, which writes tests/golden/conv_routes.json from ANOTHER build of the library).

A case is one forward or data-gradient pass through HipBackend at one shape, product mode and workspace size, run under
prof_begin() / prof_end().  Its record is {launch name: [launches, flops, bytes]}: which kernels served it, on which grid-independent
figures (the bytes of a slab_reduce_* entry carry the split count: 4 * out_elems * (ksplit + 1)).  `routes` names the enumerators of
the plan functions' route enums (csrc/vf_conv.hip: GaRoute, TrRoute, IgRoute; csrc/vf_pgemm.hip: PgRoute) the case is meant for.

Shapes are (B, Cin, H, Cout) on square maps, 4x4 stride 2 pad 1 unless `geo` says otherwise; H is the map the operand lives on
(for the transposed passes the low-resolution one)."""
import contextlib
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_routes.json")
S2, S1 = (4, 2, 1), (4, 1, 0)


def case(cid, kind, shape, routes, mode="f32_3xbf16", ws="hint", geo=S2, routing=None, bn=0, bias=True):
    return dict(id=cid, kind=kind, shape=shape, routes=routes, mode=mode, ws=ws, geo=geo, routing=routing, bn=bn, bias=bias)


# ws: "hint" (vf_workspace_bytes_hint), an integer, ("slabs", j, d): j output-sized slabs plus d bytes, or ("cols", d): the column
# buffer of the thin-output pass plus 32 MB plus d bytes
CASES = [
    # ---- planes, through pconv_gather / pconv_scatter
    case("pg/gather_m0", "gather", (2, 64, 32, 64), ["PG_PATCH_G_M0"]),
    case("pg/gather_m1", "gather", (2, 64, 16, 64), ["PG_PATCH_G_M1"]),
    case("pg/gather_m2", "gather", (8, 64, 8, 64), ["PG_PATCH_G_M2"]),
    case("pg/gather_m1_two_chunks", "gather", (2, 128, 16, 64), ["PG_PATCH_G_M1"]),      # two channel chunks on a small grid: split
    case("pg/scatter_c2", "scatter", (1, 64, 16, 64), ["PG_PATCH_TR_C2"]),
    case("pg/scatter_c4", "scatter", (64, 64, 32, 64), ["PG_PATCH_TR_C4"]),      # test_patch_fed_transposed_passes_against_the_oracle's first
    case("pg/scatter_tr_m1", "scatter", (2, 64, 8, 64), ["PG_PATCH_G_TR_M1"]),
    case("pg/scatter_tr_m2", "scatter", (8, 64, 4, 64), ["PG_PATCH_G_TR_M2"]),
    case("pg/gather_dma_64", "gather", (3, 64, 16, 64), ["PG_DMA_2STAGE"]),      # M = 192: 64-row tiles
    case("pg/gather_reg", "gather", (5, 32, 8, 96), ["PG_REG"]),
    case("pg/scatter_whole_map_512_blocks", "scatter", (32, 64, 8, 512), ["PG_DMA_1STAGE"]),
    case("pg/gather_m0_routing_off", "gather", (2, 64, 32, 64), ["PG_DMA_2STAGE"], routing=(0, 0)),
    case("pg/scatter_c2_routing_off", "scatter", (1, 64, 16, 64), ["PG_DMA_2STAGE"], routing=(0, 0)),
    case("pg/gather_bf16", "gather", (2, 64, 16, 64), ["PG_DMA_1PLANE"], mode="bf16"),
    # ---- k_igemm, through conv2d_fwd, conv2d_bwd_data, deconv2d_fwd and deconv2d_bwd_data
    case("ig/fwd_64x64_db", "fwd", (2, 64, 16, 64), ["GA_GEMM", "IG_TILE_DB"]),
    case("ig/fwd_64x64_f32", "fwd", (2, 64, 16, 64), ["GA_GEMM", "IG_TILE"], mode="f32"),
    case("ig/fwd_256x32", "fwd", (2, 64, 16, 32), ["GA_GEMM", "IG_TILE"]),
    case("ig/fwd_v0", "fwd", (2, 12, 32, 64), ["GA_GEMM", "IG_TILE"]),
    case("ig/bwd_data_kmajor_v1", "bwd_data", (2, 32, 8, 33), ["TR_PARITY_GEMM", "IG_TILE"]),      # gy with 32 channels, Cin = 33
    case("ig/fwd_128x128", "fwd", (16, 16, 64, 1024), ["GA_GEMM", "IG_TILE"]),
    case("ig/fwd_128x64", "fwd", (32, 16, 128, 64), ["GA_GEMM", "IG_TILE"]),
    case("ig/bottleneck_fwd_klin", "fwd", (16, 64, 4, 128), ["GA_GEMM", "IG_TILE_KLIN"], geo=S1),
    case("ig/full_bwd_data", "deconv_bwd_data", (2, 64, 16, 64), ["GA_GEMM", "IG_TILE_DB"]),      # gy (64, 16 x 16) -> gx (64, 8 x 8)
    # test_bottleneck_weight_streaming_threshold's pair at the smallest batch
    case("ig/smallm_rows", "fwd", (2, 512, 4, 4000), ["GA_GEMM", "IG_SMALLM_ROWS"], geo=S1),
    case("ig/smallm_kmajor", "deconv_fwd", (2, 4000, 1, 512), ["TR_GEMM_1X1", "IG_SMALLM_KMAJOR"], geo=S1),
    case("ig/full_fwd_1x1_bias", "deconv_fwd", (16, 128, 1, 64), ["TR_GEMM_1X1", "IG_TILE"], geo=S1),
    # test_thin_output_column_buffer_threshold's shape on both sides of its threshold
    case("tr/col2im", "deconv_fwd", (2, 64, 32, 12), ["TR_COL2IM", "IG_TILE_DB"], ws=("cols", 0)),
    case("tr/col2im_no_room", "deconv_fwd", (2, 64, 32, 12), ["TR_PARITY_GEMM", "IG_TILE"], ws=("cols", -4)),
    case("tr/thin_out", "deconv_fwd", (2, 128, 16, 3), ["TR_THIN_OUT"]),
    case("ga/thin_in", "fwd", (2, 3, 32, 64), ["GA_THIN_IN"]),
    case("ga/dot_head", "fwd", (2, 512, 4, 1), ["GA_DOT_HEAD"], geo=S1),
    case("tr/dot_head", "bwd_data", (2, 1, 1, 512), ["TR_DOT_HEAD"], geo=S1),      # gy (1 channel, 1 x 1) -> gx (512, 4 x 4)
    # ---- the shared split-K helper where the slabs do not fit: IGEMM_CASES[0] and PCONV_CASES[0] of tests/test_gpu_workspace.py
    case("ws/igemm_hint", "fwd", (4, 256, 8, 512), ["GA_GEMM", "IG_TILE"]),
    case("ws/igemm_two_slabs_minus_4", "fwd", (4, 256, 8, 512), ["GA_GEMM", "IG_TILE"], ws=("slabs", 2, -4)),
    case("ws/igemm_0", "fwd", (4, 256, 8, 512), ["GA_GEMM", "IG_TILE"], ws=0),
    case("ws/pconv_hint", "gather", (8, 384, 8, 128), ["PG_PATCH_G_M2"]),
    case("ws/pconv_two_slabs_minus_4", "gather", (8, 384, 8, 128), ["PG_PATCH_G_M2"], ws=("slabs", 2, -4)),
    case("ws/pconv_0", "gather", (8, 384, 8, 128), ["PG_PATCH_G_M2"], ws=0),
    # ---- one pending BatchNorm request of each mode (BN_CASES): from the slab reduce, and from the epilogue
    case("bn/fwd_slab_reduce", "fwd", (8, 128, 16, 256), ["GA_GEMM", "IG_TILE_DB"], bn=1, bias=False),
    case("bn/fwd_epilogue", "fwd", (8, 128, 16, 256), ["GA_GEMM", "IG_TILE_DB"], bn=1, bias=False, ws=0),
    case("bn/scatter_slab_reduce", "scatter", (16, 512, 4, 256), ["PG_PATCH_G_TR_M2"], bn=2, bias=False),
    case("bn/scatter_epilogue", "scatter", (16, 512, 4, 256), ["PG_PATCH_G_TR_M2"], bn=2, bias=False, ws=0),
]

# what the launch list of a case must show for an enumerator (None: that pass is not profiled under a name of its own)
ROUTE_NAMES = {
    "PG_DMA_2STAGE": r"^pconv_dma_(128|64)x64x64_t(16|4)$", "PG_DMA_1STAGE": r"^pconv_dma_128x64x64_t(16|4)_1stage$",
    "PG_DMA_1PLANE": r"^pconv_dma_(128|64)x64x64_t(16|4)_bf16$", "PG_PATCH_TR_C2": r"^pconv_patch_128x64_t4_c2$",
    "PG_PATCH_TR_C4": r"^pconv_patch_128x64_t4_c4$", "PG_PATCH_G_M0": r"^pconv_patchg_128x64_t16_m0$",
    "PG_PATCH_G_M1": r"^pconv_patchg_128x64_t16_m1$", "PG_PATCH_G_M2": r"^pconv_patchg_128x64_t16_m2$",
    "PG_PATCH_G_TR_M1": r"^pconv_patchg_128x64_t4_m1$", "PG_PATCH_G_TR_M2": r"^pconv_patchg_128x64_t4_m2$",
    "PG_REG": r"^pconv_(128|64)x64x(32|64)_t(16|4)$",
    "IG_TILE": r"^igemm_\d+x\d+_(rowB|kmajorB)_v[012](_bf16x3|_bf16)?$", "IG_TILE_KLIN": r"^igemm_64x128_rowB_v2(_bf16x3|_bf16)?$",
    "IG_TILE_DB": r"^igemm_64x64_(rowB|kmajorB)_v2_bf16x3_db$", "IG_SMALLM_ROWS": r"^smallm_rowdot$", "IG_SMALLM_KMAJOR": r"^smallm_axpy$",
    "GA_GEMM": r"^(igemm_|smallm_)", "GA_THIN_IN": r"^conv_thin_in$", "GA_DOT_HEAD": None,
    "TR_PARITY_GEMM": r"^igemm_", "TR_GEMM_1X1": r"^(igemm_|smallm_)", "TR_COL2IM": r"^col2im4x4$", "TR_THIN_OUT": r"^deconv_thin_out$",
    "TR_DOT_HEAD": None,
}


def route_enumerators():
    """every enumerator of the route enums, read from the sources the library is built from"""
    out = []
    for src, enums in (("vf_conv.hip", ("GaRoute", "TrRoute", "IgRoute")), ("vf_pgemm.hip", ("PgRoute",))):
        text = open(os.path.join(ROOT, "video-filler_amd", "csrc", src)).read()
        for e in enums:
            body = re.search(r"enum %s \{(.*?)\};" % e, text, re.S).group(1)
            out += re.findall(r"^\s*([A-Z][A-Z0-9_]+)\b", re.sub(r"//[^\n]*", "", body), re.M)
    return out


def _rand(b, seed, shape, scale=1.0):
    """seeded values on the device, logical NCHW / physical NHWC"""
    g = torch.Generator(device=b.device).manual_seed(seed)
    n, c, h, w = shape
    return (torch.randn((n, h, w, c), generator=g, device=b.device) * scale).permute(0, 3, 1, 2)


def _zeros(b, shape):
    n, c, h, w = shape
    return torch.zeros((n, h, w, c), device=b.device).permute(0, 3, 1, 2)


@contextlib.contextmanager
def _workspace(b, nbytes):
    import ctypes as C
    from video_filler_amd import _lib
    buf = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=b.device)
    old = b.workspace
    _lib.check(b.lib.vf_ctx_set_workspace(b.ctx, C.c_void_p(buf.data_ptr()), nbytes))
    b.workspace = buf[:nbytes]
    try:
        yield
    finally:
        b.synchronize()
        b.workspace = old
        _lib.check(b.lib.vf_ctx_set_workspace(b.ctx, C.c_void_p(old.data_ptr()), old.numel()))


def run_case(b, c):
    """-> (record {name: [launches, flops, bytes]}, the tensors the pass wrote).  b: a HipBackend of the caller's own"""
    B, Cin, H, Cout = c["shape"]
    k, s, p = c["geo"]
    kind, seed = c["kind"], 1 + 16 * [x["id"] for x in CASES].index(c["id"])
    b.set_mfma_mode(c["mode"])
    if c["routing"] is not None:
        b.pconv_set_routing(*c["routing"])
    try:
        Hd, Hu = (H + 2 * p - k) // s + 1, (H - 1) * s - 2 * p + k      # the map below / above the operand's
        x = _rand(b, seed, (B, Cin, H, H))
        bias = _rand(b, seed + 2, (1, Cout, 1, 1), 0.1).reshape(Cout) if c["bias"] else None
        if kind in ("fwd", "gather"):
            w, y = _rand(b, seed + 1, (Cout, Cin, k, k), 0.05), _zeros(b, (B, Cout, Hd, Hd))
        elif kind == "deconv_bwd_data":      # x: gradOutput of a full-conv Cout -> Cin
            w, y, bias = _rand(b, seed + 1, (Cout, Cin, k, k), 0.05), _zeros(b, (B, Cout, Hd, Hd)), None
        elif kind == "bwd_data":             # x: gradOutput of a conv Cout -> Cin
            w, y, bias = _rand(b, seed + 1, (Cin, Cout, k, k), 0.05), _zeros(b, (B, Cout, Hu, Hu)), None
        else:                                # deconv_fwd, scatter: full-conv weight [Cin][Cout]
            w, y = _rand(b, seed + 1, (Cin, Cout, k, k), 0.05), _zeros(b, (B, Cout, Hu, Hu))
        if kind == "gather":
            xp, wp = b.planes_split(x), b.weight_planes(w, want_transposed=False)[0]
        elif kind == "scatter":
            xp, wp = b.planes_split(x), b.weight_planes(w)[1]
        written = [y]
        part = None
        if c["bn"]:
            part = torch.zeros(1024 * 2 * Cout, dtype=torch.float64, device=b.device)
            written.append(part)
        if c["bn"] == 1:
            shift = _rand(b, seed + 3, (1, Cout, 1, 1), 0.1).reshape(Cout)
        elif c["bn"] == 2:
            bx, yact = _rand(b, seed + 3, tuple(y.shape)), _rand(b, seed + 4, tuple(y.shape))
            mean = _rand(b, seed + 5, (1, Cout, 1, 1), 0.1).reshape(Cout)

        def go():
            if c["bn"] == 1:
                b.bn_fuse_next_fwd(shift, part, 1)
            elif c["bn"] == 2:
                b.bn_fuse_next_bwd(bx, yact, "lrelu", 0.2, mean, part, 1)
            if kind == "fwd":
                b.conv2d_fwd(x, w, bias, y, k, s, p, "lrelu", 0.2)
            elif kind == "bwd_data":
                b.conv2d_bwd_data(x, w, y, k, s, p)
            elif kind == "deconv_fwd":
                b.deconv2d_fwd(x, w, bias, y, k, s, p, "relu", 0.0)
            elif kind == "deconv_bwd_data":
                b.deconv2d_bwd_data(x, w, y, k, s, p)
            elif kind == "gather":
                b.pconv_gather(xp, wp, bias, y, B, H, H, Cin, Cout, "lrelu", 0.2)
            else:
                b.pconv_scatter(xp, wp, bias, y, B, H, H, Cin, Cout)

        ws = c["ws"]
        if ws == "hint":
            ws = int(b.lib.vf_workspace_bytes_hint())
        elif isinstance(ws, (tuple, list)) and ws[0] == "slabs":
            ws = ws[1] * 4 * y.numel() + ws[2]
        elif isinstance(ws, (tuple, list)):
            ws = B * H * H * 16 * Cout * 4 + (32 << 20) + ws[1]
        with _workspace(b, ws):
            b.prof_begin()
            try:
                go()
            finally:
                prof = b.prof_end()
            rows = b.bn_fuse_result() if c["bn"] else None
        rec = {n: [int(e["launches"]), float(e["flops"]), float(e["bytes"])] for n, e in sorted(prof.items())}
        if rows is not None:
            rec["bn_fuse_result"] = [int(rows), 0.0, 0.0]
        return rec, written
    finally:
        b.set_mfma_mode("f32_3xbf16")
        if c["routing"] is not None:
            b.pconv_set_routing(1, 1)


def check_routes(c, rec):
    """the launch list shows what the case's enumerators stand for"""
    names = [n for n in rec if not n.startswith("slab_reduce_") and n != "bn_fuse_result"]
    for r in c["routes"]:
        pat = ROUTE_NAMES[r]
        if pat is None:
            assert not names, "%s: %s launches nothing under a profiled name, got %s" % (c["id"], r, names)
        else:
            assert any(re.search(pat, n) for n in names), "%s: no launch of %s among %s" % (c["id"], r, names)
