"""timing of the image-side conv forward (3 input channels): direct kernel vs the implicit-GEMM scalar path (VF_NO_THIN=1)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from video_filler_amd.backend import get_backend
hb = get_backend()
def timeit(fn, nb=30):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(nb): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / nb * 1e3
for Bn, H in ((64, 128), (128, 64)):
    x = hb.empty_act(Bn, 3, H, H).normal_()
    y = hb.empty_act(Bn, 64, H // 2, H // 2)
    w = (hb.empty(64, 4, 4, 3).normal_() * 0.02).permute(0, 3, 1, 2)
    b = hb.zeros(64)
    yp = torch.empty((3, y.numel()), dtype=torch.bfloat16, device=hb.device)
    print("B=%d H=%d: conv2d_fwd %.1f us   conv2d_fwd_planes %.1f us   planes_split alone %.1f us" % (
        Bn, H, timeit(lambda: hb.conv2d_fwd(x, w, b, y, 4, 2, 1, "lrelu", 0.2)),
        timeit(lambda: hb.conv2d_fwd_planes(x, w, b, y, yp, 4, 2, 1, "lrelu", 0.2)), timeit(lambda: hb.planes_split(y, yp))))

# ---- the generator's last full-conv (64 -> 3) seen from its output: its data-gradient is a 3 -> 64 channel conv of the image gradient
# whose epilogue also reads the BatchNorm input and the activated BatchNorm output below (mask + backward sums).  Three timings at the
# workload's shape: today's route with the request, the direct thin kernel on the same conv WITHOUT any epilogue, and a streaming
# pass with exactly the epilogue's memory traffic (vf_act_bwd: two tensors of the output's size read, one written) — the least any
# kernel that carries the epilogue can take beyond its input
Bn, Hl = 64, 64
gimg = hb.empty_act(Bn, 3, 2 * Hl, 2 * Hl).normal_()                  # gradient of the 128 x 128 image
wfull = (hb.empty(64, 4, 4, 3).normal_() * 0.02).permute(0, 3, 1, 2)  # full-conv weight [Cin = 64][kh][kw][Cout = 3]
gx = hb.empty_act(Bn, 64, Hl, Hl)
xbn = hb.empty_act(Bn, 64, Hl, Hl).normal_()
yact = torch.relu(xbn.clone())
mean = hb.zeros(64)
part = torch.zeros((Bn * Hl * Hl // 64 + 8, 2 * 64), dtype=torch.float64, device=hb.device)      # the net object's own row cap
def dx_fused():
    hb.bn_fuse_next_bwd(xbn, yact, "relu", 0.0, mean, part)
    hb.deconv2d_bwd_data(gimg, wfull, gx, 4, 2, 1)
    return hb.bn_fuse_result()
rows = dx_fused()
hb.prof_begin(); dx_fused(); names = sorted(hb.prof_end())
t_fused = timeit(dx_fused)
t_thin = timeit(lambda: hb.conv2d_fwd(gimg, wfull, None, gx, 4, 2, 1, "none", 0.0))
t_floor = timeit(lambda: hb.act_bwd(yact, xbn, gx, "relu", 0.0))
print("last full-conv dX, B=64, 64x64 low-res: with BatchNorm-backward epilogue %.1f us (%s, %d partial rows)   thin kernel, no epilogue %.1f us"
      "   epilogue traffic alone (201 MB streamed) %.1f us" % (t_fused, " ".join(names), rows, t_thin, t_floor))
