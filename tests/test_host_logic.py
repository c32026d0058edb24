"""Host-side logic of the package on CPU (no GPU needed): the nn mirror, the Sequential fusion plan, the flat
parameter layout, the trainers' closures and the data-parallel path, driven through tests/oracle_backend.py
(an oracle-backed stand-in for the HIP backend that only tests may install)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import video_filler_amd  # noqa: F401
from video_filler_amd import backend as vb

from helpers import rel_err
from oracle_backend import OracleBackend

SMALL = dict(nBottleneck=32, nef=8, ngf=8, ndf=8)


@pytest.fixture()
def cpu_backend():
    old = vb._BACKEND
    b = vb.set_backend(OracleBackend())
    yield b
    vb._BACKEND = old


def _load(tr, ref):
    tr.netG.load_reference_flat(torch.from_numpy(ref.parametersG.copy()))
    tr.netD.load_reference_flat(torch.from_numpy(ref.parametersD.copy()))


def test_fusion_plan_and_module_protocol(cpu_backend):
    from video_filler_amd import nn
    from video_filler_amd.trainers import build_netD, build_netG
    netD = build_netD(3, 8, False)
    kinds = [(type(m).__name__, type(a).__name__ if a else None) for m, a in netD._build_plan()]
    assert kinds == [("SpatialConvolution", "LeakyReLU"),
                     ("SpatialConvolution", None), ("SpatialBatchNormalization", "LeakyReLU"),
                     ("SpatialConvolution", None), ("SpatialBatchNormalization", "LeakyReLU"),
                     ("SpatialConvolution", None), ("SpatialBatchNormalization", "LeakyReLU"),
                     ("SpatialConvolution", "Sigmoid"), ("View", None)]
    netG = build_netG(3, 3, 8, 8, 32, False)
    assert len(netG.leaves()) == 31                                   # train.lua:87-148: 15 (netE) + 2 + 4*3 + 2
    assert sum(isinstance(m, nn.SpatialBatchNormalization) for m in netG.leaves()) == 9
    unf = build_netD(3, 8, False, fuse=False)
    assert all(a is None for _, a in unf._build_plan())
    # torch.type(m):find('Convolution') semantics used by weights_init / the bias-zeroing sweep (train.lua:58-67,279)
    names = [m.type_name() for m in netG.leaves()]
    assert sum("Convolution" in n for n in names) == 11 and sum("BatchNormalization" in n for n in names) == 9
    m = netG.leaves()[0]
    assert (m.nInputPlane, m.nOutputPlane, m.kW, m.kH, m.dW, m.dH, m.padW, m.padH) == (3, 8, 4, 4, 2, 2, 1, 1)


def test_parameter_counts_match_the_reference_nets(cpu_backend):
    """train.lua netD has 2 766 529 parameters; netG (nBottleneck=100) 7.22 M."""
    from video_filler_amd.trainers import build_netD, build_netG
    netD = build_netD(3, 64, False)
    netD.getParameters()
    assert netD.n_parameters() == 2766529
    netG = build_netG(3, 3, 64, 64, 100, False)
    netG.getParameters()
    n = netG.n_parameters()
    assert abs(n - 7.22e6) < 0.01e6
    vidD = build_netD(12, 64, True)
    vidD.getParameters()
    assert vidD.n_parameters() == 2802401          # train_vid_weighted.lua netD, predLen = 4


def test_flat_layout_alignment_views_and_roundtrip(cpu_backend):
    from video_filler_amd.trainers import build_netG
    net = build_netG(3, 3, 8, 8, 32, True)
    flat, gflat = net.getParameters()
    rng = np.random.default_rng(0)
    ref = rng.standard_normal(net.n_parameters()).astype(np.float32)
    net.load_reference_flat(torch.from_numpy(ref))
    np.testing.assert_array_equal(net.reference_flat().numpy(), ref)
    for m, name, gname, o, n in net._flat[2]:
        assert o % 64 == 0                                           # 256-byte aligned segments
        t = getattr(m, name)
        assert t.data_ptr() == flat.data_ptr() + 4 * o                # a VIEW into the flat storage
        if t.dim() == 4:
            assert t.permute(0, 2, 3, 1).is_contiguous()              # channels-last physical layout
    # padding between segments stays zero
    used = torch.zeros_like(flat, dtype=torch.bool)
    for m, name, gname, o, n in net._flat[2]:
        used[o:o + n] = True
    assert float(flat[~used].abs().sum()) == 0.0
    # bias zeroing sweep touches conv/full-conv biases only
    flat.fill_(1.0)
    net.zeroConvBiases()
    for m, name, gname, o, n in net._flat[2]:
        want = 0.0 if (name == "bias" and "Convolution" in m.type_name()) else 1.0
        assert float(flat[o:o + n].min()) == float(flat[o:o + n].max()) == want


def test_lazy_zero_equals_memset(cpu_backend):
    from video_filler_amd.trainers import CenterTrainer
    from oracle import oracle as O
    batch = torch.from_numpy(O.synth_center_batch(2, np.random.default_rng(3)))
    out = []
    for lazy in (True, False):
        tr = CenterTrainer(dict(SMALL, wtl2=0.999, overlapPred=4), seed=5, lazy_zero=lazy)
        tr.gradParametersD.fill_(7.0)      # stale garbage must not leak into the new gradients
        tr.gradParametersG.fill_(7.0)
        tr.set_batch(batch)
        tr.step()
        out.append((tr.netD.reference_flat(grads=True).numpy().copy(), tr.netG.reference_flat(grads=True).numpy().copy()))
    assert rel_err(out[0][0], out[1][0]) < 1e-6 and rel_err(out[0][1], out[1][1]) < 1e-6


def test_exchange_ranges_leave_out_the_fused_slices(cpu_backend):
    """the data-parallel step all-reduces everything BUT the slices whose operands are gathered (trainers._exchange_ranges); on
    this backend (the mirror host) nothing is fused and the whole bucket travels"""
    from video_filler_amd.trainers import CenterTrainer
    tr = CenterTrainer(dict(SMALL, wtl2=0.999, overlapPred=4), seed=5)
    assert tr.fuse_adam == "on" and tr.fuse_adam_slices() == [] and tr.fused_adam_ranges() == []
    assert tr._exchange_ranges(0, 50) == [(0, 50)]
    tr._dpf = [(30, 40), (10, 20)]
    assert tr._exchange_ranges(0, 50) == [(0, 10), (20, 30), (40, 50)]
    assert tr._exchange_ranges(15, 35) == [(20, 30)]
    assert tr._exchange_ranges(10, 20) == [] and tr._exchange_ranges(40, 50) == [(40, 50)]
    assert tr._exchange_ranges(0, 10) == [(0, 10)] and tr._exchange_ranges(12, 18) == []
    tr._dpf = []


def test_gradient_buckets_and_split_backward(cpu_backend):
    """Data-parallel bucketing: the tail bucket (bottleneck conv + decoder) owns > 90 % of netG's gradient bytes and is
    final after the upper part of the backward walk; the cut walk equals the uncut one."""
    from video_filler_amd.trainers import CenterTrainer
    from video_filler_amd import nn
    from oracle import oracle as O
    batch = torch.from_numpy(O.synth_center_batch(3, np.random.default_rng(3)))
    opt = dict(SMALL, nBottleneck=512, wtl2=0.999, overlapPred=4)     # bottleneck-dominated, like the real nets
    tr = CenterTrainer(opt, seed=5)
    k, off = tr.netG.bucket_split()
    m = tr.netG._plan[k][0]
    assert isinstance(m, nn.SpatialConvolution) and m.dW == 1 and m.nOutputPlane == 512
    n = tr.gradParametersG.numel()
    assert 0 < off < n and (n - off) >= 0.9 * tr.netG.n_parameters()
    tr.set_batch(batch)
    tr.step()
    whole = tr.gradParametersG.clone()
    # the same fGx with the pass cut at the bucket boundary (what _phase_b / _phase_b2 do)
    tr2 = CenterTrainer(opt, seed=5)
    tr2.set_batch(batch)
    tr2._phase_a()
    tr2._phase_b()
    tail_after_b = tr2.gradParametersG[off:].clone()
    tr2._phase_b2()
    assert torch.equal(tail_after_b, tr2.gradParametersG[off:])          # B2 does not touch the tail bucket
    assert torch.equal(tr2.gradParametersG, whole)


@pytest.mark.parametrize("fuse,batch_d", [(True, False), (False, False), (True, True), (False, True)])
def test_center_trainer_closures_match_oracle(fuse, batch_d, cpu_backend):
    """batch_d: netD's real and fake passes as one batch of 2B, BatchNorm in two groups — the same closures."""
    from video_filler_amd.trainers import CenterTrainer
    from oracle import oracle as O
    opt = dict(SMALL, wtl2=0.999, overlapPred=4)
    ref = O.CenterTrainer(opt, np.random.default_rng(1))
    tr = CenterTrainer(opt, fuse=fuse, lazy_zero=fuse, skip_dead_grads=fuse)
    tr.set_batch_d(batch_d)
    _load(tr, ref)
    for it in range(2):
        batch = O.synth_center_batch(2, np.random.default_rng(30 + it))
        ref.set_batch(batch)
        tr.set_batch(torch.from_numpy(batch))
        ref.step()
        tr.step()
        got = tr.losses()
        for k in ("errD", "errG", "errG_l2"):
            assert abs(got[k] - getattr(ref, k)) < 1e-5 * max(1, abs(getattr(ref, k)))
        assert rel_err(tr.netD.reference_flat(grads=True).numpy(), ref.gradParametersD) < 2e-5
        assert rel_err(tr.netG.reference_flat(grads=True).numpy(), ref.gradParametersG) < 2e-5
        sel = np.abs(ref.gradParametersG) > 1e-3 * np.abs(ref.gradParametersG).max()
        assert np.abs(tr.netG.reference_flat().numpy() - ref.parametersG)[sel].max() < 0.02 * 0.002


@pytest.mark.parametrize("variant", ["conditionAdv", "noiseGen", "both_drawn_noise"])
def test_center_trainer_option_branches_match_oracle(variant, cpu_backend):
    """train.lua's conditionAdv (table-input netD: ParallelTable of two 5x5 convs + JoinTable, df_dg[2]) and noiseGen
    (table-input netG with the 1x1 noise conv) closures through the nn mirror against the oracle's restatement."""
    from video_filler_amd.trainers import CenterTrainer
    from video_filler_amd import nn
    from oracle import oracle as O
    opt = dict(SMALL, wtl2=0.999, overlapPred=4, nz=12, conditionAdv=variant != "noiseGen", noiseGen=variant != "conditionAdv")
    ref = O.CenterTrainer(opt, np.random.default_rng(1))
    tr = CenterTrainer(opt, seed=77)
    ref.noise_seed = 77
    assert not tr.batch_d or not opt["conditionAdv"]
    if opt["conditionAdv"]:
        assert isinstance(tr.netD.modules[0], nn.ParallelTable) and isinstance(tr.netD.modules[1], nn.JoinTable)
        assert tr.netD.modules[0].modules[1].modules[0].padH == 34
    if opt["noiseGen"]:
        assert isinstance(tr.netG.modules[0], nn.ParallelTable)
    _load(tr, ref)
    for it in range(1):     # one iteration: Adam's first steps amplify 1e-7 gradient noise on these tiny nets (the GPU
        # suite runs two iterations with the whole optimizer state carried over from the oracle in between)
        batch = O.synth_center_batch(2, np.random.default_rng(40 + it))
        if variant == "noiseGen":
            noise = np.random.default_rng(50 + it).standard_normal((2, 12, 1, 1)).astype(np.float32)
            ref.set_noise(noise)
            tr.set_noise(torch.from_numpy(noise))
        ref.set_batch(batch)
        tr.set_batch(torch.from_numpy(batch))
        ref.step()
        tr.step()
        got = tr.losses()
        for k in ("errD", "errG", "errG_l2"):
            assert abs(got[k] - getattr(ref, k)) < 1e-5 * max(1, abs(getattr(ref, k))), k
        assert rel_err(tr.netD.reference_flat(grads=True).numpy(), ref.gradParametersD) < 2e-5
        assert rel_err(tr.netG.reference_flat(grads=True).numpy(), ref.gradParametersG) < 2e-5
        assert tr.netD.reference_flat().numel() == ref.parametersD.size
        assert tr.netG.reference_flat().numel() == ref.parametersG.size
        sel = np.abs(ref.gradParametersG) > 1e-3 * np.abs(ref.gradParametersG).max()
        assert np.abs(tr.netG.reference_flat().numpy() - ref.parametersG)[sel].max() < 0.02 * 0.002


@pytest.mark.parametrize("batch_d", [False, True])
@pytest.mark.parametrize("variant", ["weighted", "nomask0_gdl"])
def test_vid_trainer_closures_match_oracle(variant, batch_d, cpu_backend):
    from video_filler_amd.trainers import VidTrainer
    from oracle import oracle as O
    opt = dict(SMALL, predLen=2) if variant == "weighted" else dict(SMALL, predLen=1, weight_nomask=0, wtgdl=0.5)
    nc = 6 if variant == "weighted" else 3
    ref = O.VidTrainer(opt, np.random.default_rng(2))
    tr = VidTrainer(opt)
    tr.set_batch_d(batch_d)
    _load(tr, ref)
    ctx, full, mask = O.synth_vid_batch(3, np.random.default_rng(9), nc)
    ref.set_batch(ctx, full, mask)
    tr.set_batch(torch.from_numpy(ctx), torch.from_numpy(full), torch.from_numpy(mask))
    ref.step()
    tr.step()
    got = tr.losses()
    for k in ("errD", "errG", "errG_l2", "errG_gdl"):
        want = getattr(ref, k)
        if want is not None:
            assert abs(got[k] - want) < 1e-5 * max(1, abs(want)), k
    assert rel_err(tr.netD.reference_flat(grads=True).numpy(), ref.gradParametersD) < 2e-5
    assert rel_err(tr.netG.reference_flat(grads=True).numpy(), ref.gradParametersG) < 2e-5


@pytest.mark.parametrize("variant", ["logoNet", "withInit", "ext256"])
def test_vid_trainer_option_branches_match_oracle(variant, cpu_backend):
    """train_logo_withmask.lua's generator (last decoder stage ngf -> ngf/2) and train_vid_weighted.lua's withInit path
    (initializer net in training mode, inpaint_utils.fillIn, then the usual closures); ext256: the labelled fineSize-256
    extension (one more stride-2 stage in netD and on either side of netG's bottleneck — the reference's own netD fails at
    that size, SURVEY D5, so this is parity with the oracle's same extension, not with the reference)."""
    from video_filler_amd.trainers import VidTrainer, build_netG
    from oracle import oracle as O
    fs = 128
    if variant == "logoNet":
        opt = dict(SMALL, predLen=1, weight_nomask=1, wtgdl=0, logoNet=True)
    elif variant == "ext256":
        opt = dict(SMALL, predLen=1, fineSize=256, ext256=True, wtgdl=0.5)
        fs = 256
        with pytest.raises(AssertionError, match="ext256"):
            VidTrainer(dict(opt, ext256=False))
    else:
        opt = dict(SMALL, predLen=1)
    ref = O.VidTrainer(opt, np.random.default_rng(2))
    tr = VidTrainer(opt)
    if variant == "logoNet":
        assert tr.netG.leaves()[-2].nInputPlane == SMALL["ngf"] // 2
    elif variant == "ext256":
        assert len([m for m in tr.netD.leaves() if m.type_name() == "nn.SpatialConvolution"]) == 7
        assert len([m for m in tr.netG.leaves() if "Convolution" in m.type_name()]) == 14      # 7 + 7 (one more on each side)
    else:
        rI = O.build_netG(3, 3, 8, 8, 16, True)
        O.weights_init(rI, np.random.default_rng(8))
        pI, _ = rI.getParameters()
        hI = build_netG(3, 3, 8, 8, 16, True)
        hI.getParameters()
        hI.load_reference_flat(torch.from_numpy(pI.copy()))
        ref.netI = rI
        tr.set_initializer(hI)
    _load(tr, ref)
    ctx, full, mask = O.synth_vid_batch(3, np.random.default_rng(9), 3, fineSize=fs)
    ref.set_batch(ctx, full, mask)
    tr.set_batch(torch.from_numpy(ctx), torch.from_numpy(full), torch.from_numpy(mask))
    ref.step()
    tr.step()
    got = tr.losses()
    for k in ("errD", "errG", "errG_l2"):
        want = getattr(ref, k)
        assert abs(got[k] - want) < 1e-5 * max(1, abs(want)), k
    assert rel_err(tr.netD.reference_flat(grads=True).numpy(), ref.gradParametersD) < 2e-5
    assert rel_err(tr.netG.reference_flat(grads=True).numpy(), ref.gradParametersG) < 2e-5
    if variant == "withInit":
        np.testing.assert_array_equal(tr.input_ctx.numpy(), ctx)          # the loader's batch is left intact
        assert rel_err(tr._ctx_filled.numpy(), ref.input_ctx) < 1e-6
        rb = [m for m in rI.modules[0].modules if hasattr(m, "running_mean")][0]
        hb = [m for m in hI.leaves() if hasattr(m, "running_mean")][0]
        assert rel_err(hb.running_mean.numpy(), rb.running_mean) < 1e-5    # netI ran in training mode on both sides


def test_checkpoint_roundtrip(tmp_path, cpu_backend):
    from video_filler_amd import util
    from video_filler_amd.trainers import build_netG, weights_init
    a = build_netG(3, 3, 8, 8, 32, False)
    weights_init(a, torch.Generator().manual_seed(1))
    a.getParameters()
    for m in a.leaves():
        if hasattr(m, "running_mean"):
            m.running_mean.uniform_(-1, 1)
            m.running_var.uniform_(0.5, 2)
    f = str(tmp_path / "net_G.npz")
    util.save(f, a)
    b = util.load(f, build_netG(3, 3, 8, 8, 32, False))
    np.testing.assert_array_equal(a.reference_flat().numpy(), b.reference_flat().numpy())
    ra = [m.running_var.numpy() for m in a.leaves() if hasattr(m, "running_var")]
    rb = [m.running_var.numpy() for m in b.leaves() if hasattr(m, "running_var")]
    assert len(ra) == 9 and all(np.array_equal(x, y) for x, y in zip(ra, rb))
    assert util.cudnn(a) is a          # drivers keep their util.cudnn(net) call


# ------------------------------------------------------------------ data parallel over gloo, world_size 2 and 4
def _dp_worker(rank, world, port, kind, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from oracle import oracle as O
    from video_filler_amd import backend as vb2
    from video_filler_amd.trainers import CenterTrainer, VidTrainer
    vb2.set_backend(OracleBackend())
    local_bn = kind.endswith("_local")           # sync_bn=False: every rank normalises with its own shard's statistics
    shard = kind.endswith("_shard")              # shard_adam: reduce-scatter G's gradient, Adam on 1 / world of it, all-gather
    base = kind[:-len("_local")] if local_bn else (kind[:-len("_shard")] if shard else kind)
    B = 2 * world
    if base.startswith("center"):
        opt = dict(SMALL, wtl2=0.999, overlapPred=4, smooth=True)   # smooth nets: see tests/test_gpu_trainers.py
        full_batch = torch.from_numpy(O.synth_center_batch(B, np.random.default_rng(77)))
        mk = lambda w, r, s: CenterTrainer(opt, seed=11, world=w, rank=r, sync_bn=s, shard_adam=shard and w > 1)
        feed = lambda tr, lo, hi: tr.set_batch(full_batch[lo:hi])
    else:
        opt = dict(SMALL, predLen=2, smooth=True)
        ctx, full, mask = [torch.from_numpy(a) for a in O.synth_vid_batch(B, np.random.default_rng(78), 6)]
        mk = lambda w, r, s: VidTrainer(opt, seed=11, world=w, rank=r, sync_bn=s, shard_adam=shard and w > 1)
        feed = lambda tr, lo, hi: tr.set_batch(ctx[lo:hi], full[lo:hi], mask[lo:hi])
    tr = mk(world, rank, not local_bn)
    per = B // world
    # "vid" runs the phased step (A | all-reduce D | B | all-reduce G | C) that bench.py uses for N > 1;
    # "center" runs the plain loop body with the exchange inside the closures.  Both must equal the big batch.
    # "*_pipe" runs the pipelined step (G's exchange and Adam deferred behind the next iteration's netD real pass).
    if base.endswith("_pipe"):
        tr._pipelined = True
        dp_step = tr.step_pipelined
    else:
        dp_step = tr.step_phased if (base == "vid" or shard) else tr.step
    feed(tr, rank * per, (rank + 1) * per)
    dp_step()
    g1 = tr.gradParametersG.numpy().copy()      # after ONE iteration: gradients are comparable at fp32 precision
    gD1 = tr.gradParametersD.numpy().copy()
    rm1 = [m.running_mean.numpy().copy() for m in tr.netG.leaves() if hasattr(m, "running_mean")]
    feed(tr, rank * per, (rank + 1) * per)
    dp_step()
    tr.flush()                                  # pipelined: the last iteration's Adam(G) is still pending
    res = dict(pG=tr.parametersG.numpy().copy(), pD=tr.parametersD.numpy().copy(), gG=g1, rm=rm1)
    if rank == 0 and not local_bn:
        one = mk(1, 0, False)                 # the single-device big batch the shards must reproduce
        feed(one, 0, B)
        one.step()
        one_g1 = one.gradParametersG.numpy().copy()
        one_rm1 = [m.running_mean.numpy().copy() for m in one.netG.leaves() if hasattr(m, "running_mean")]
        feed(one, 0, B)
        one.step()
        ok = dict(pG=rel_err(res["pG"], one.parametersG.numpy()), pD=rel_err(res["pD"], one.parametersD.numpy()),
                  gG=rel_err(res["gG"], one_g1),
                  rm=max(float(np.abs(a - b).max()) for a, b in zip(res["rm"], one_rm1)))
        np.save(os.path.join(out_dir, "ok.npy"), np.array([ok["pG"], ok["pD"], ok["gG"], ok["rm"]]))
    if rank == 0 and local_bn:
        # local statistics: the exchanged gradient is the MEAN over ranks of what a single-device trainer computes on each
        # shard alone (same initial weights; netD's gradient does not depend on netG's update, netG's is taken after the
        # averaged Adam(D) step — so replay D's update with the mean gradient before each shard's fGx)
        gD, gG, rms = [], [], []
        shard = []
        for r in range(world):
            one = mk(1, 0, False)
            feed(one, r * per, (r + 1) * per)
            one.fDx(one.parametersD)
            gD.append(one.gradParametersD.numpy().copy())
            shard.append(one)
        gD_mean = np.mean(np.stack(gD), axis=0, dtype=np.float64).astype(np.float32)
        from video_filler_amd import optim as vopt
        for one in shard:
            one.gradParametersD.copy_(torch.from_numpy(gD_mean))
            vopt.adam_update(one.parametersD, one.gradParametersD, one.optimStateD)
            one.fGx(one.parametersG)
            gG.append(one.gradParametersG.numpy().copy())
        gG_mean = np.mean(np.stack(gG), axis=0, dtype=np.float64).astype(np.float32)
        rm_own = [m.running_mean.numpy().copy() for m in shard[0].netG.leaves() if hasattr(m, "running_mean")]
        ok = dict(gD=rel_err(gD1, gD_mean), gG=rel_err(g1, gG_mean),
                  rm=max(float(np.abs(a - b).max()) for a, b in zip(rm1, rm_own)))
        np.save(os.path.join(out_dir, "ok.npy"), np.array([0.0, ok["gD"], ok["gG"], ok["rm"]]))
    # replicas must stay bit-identical across ranks
    t = torch.from_numpy(res["pG"]).clone()
    dist.broadcast(t, 0)
    same = bool(torch.equal(t, torch.from_numpy(res["pG"])))
    flag = torch.tensor([1.0 if same else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        np.save(os.path.join(out_dir, "same.npy"), flag.numpy())
    dist.destroy_process_group()


def _dp_rows_worker(rank, world, port, mode, out_dir):
    """the phased data-parallel step with the bottleneck pair's update SHARDED BY WEIGHT ROWS (trainer.dp_fused = "rows", the default) or
    formed on every rank ("gathered"), on the module-by-module host with the fused-Adam protocol's test double
    (oracle_backend.install_fused_adam_emulation): which slices stay out of the exchange, the row blocks (32 rows: 16 / 16 at two
    ranks, a ragged 12 / 12 / 8 at three), the exchange of the updated blocks deferred into the next iteration, flush(), the marks on
    the optimiser state — against the single-device big batch."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from oracle import oracle as O
    from oracle_backend import install_fused_adam_emulation
    from video_filler_amd import backend as vb2
    from video_filler_amd.trainers import VidTrainer
    vb2.set_backend(OracleBackend())
    install_fused_adam_emulation()
    B = 2 * world
    opt = dict(SMALL, predLen=2, smooth=True)
    ctx, full, mask = [torch.from_numpy(a) for a in O.synth_vid_batch(B, np.random.default_rng(78), 6)]
    mk = lambda w, r: VidTrainer(opt, seed=11, world=w, rank=r, sync_bn=w > 1)
    feed = lambda tr, lo, hi: tr.set_batch(ctx[lo:hi], full[lo:hi], mask[lo:hi])
    tr = mk(world, rank)
    tr.dp_fused = mode
    per = B // world
    checks = []
    for it in range(3):
        feed(tr, rank * per, (rank + 1) * per)
        tr.step_phased()
        if it == 0:
            slices = tr.fused_adam_ranges() if hasattr(tr, "fused_adam_ranges") else []
            checks.append(len(tr._dpf) == 2)                                     # the pair was left to the fused update ...
            checks.append(all(float(tr.gradParametersG[lo:hi].abs().max()) == 0.0 for lo, hi in tr._dpf))      # ... and not exchanged
    if mode == "rows":
        blocks = [[hi - lo for lo, hi in per_rank] for per_rank in tr._row_ranges]
        checks.append(tr._rows_stale and tr.optimStateG.get("row_shard") == (rank, world))
        checks.append(all(sum(b) == hi - lo for b, (lo, hi) in zip(blocks, tr._dpf)))
        if world == 3:
            checks.append(all(len(set(b)) == 2 and b[0] == b[1] > b[2] > 0 for b in blocks))      # ragged: 12 / 12 / 8 rows
        else:
            checks.append(all(len(set(b)) == 1 for b in blocks))
        before = tr.parametersG.clone()
        tr.flush()                                                               # the exchange the next iteration would have opened with
        checks.append(not tr._rows_stale and not torch.equal(before, tr.parametersG))
        try:                                                                     # a sharded Adam state refuses another mode
            tr.dp_fused = "gathered"
            feed(tr, rank * per, (rank + 1) * per)
            tr.step_phased()
            checks.append(False)
        except RuntimeError as e:
            checks.append("gather_adam_state" in str(e))
        tr.dp_fused = "rows"
        tr._dpf = []
        tr.netG.set_fused_adam(False)
        tr.gather_adam_state()
        checks.append("row_shard" not in tr.optimStateG)
    else:
        checks.append(not tr._rows_stale and "row_shard" not in tr.optimStateG)
    res = dict(pG=tr.parametersG.numpy().copy(), pD=tr.parametersD.numpy().copy(), m=tr.optimStateG["m"].numpy().copy())
    if rank == 0:
        one = mk(1, 0)
        for it in range(3):
            feed(one, 0, B)
            one.step()
        np.save(os.path.join(out_dir, "ok.npy"), np.array([rel_err(res["pG"], one.parametersG.numpy()), rel_err(res["pD"], one.parametersD.numpy()),
                                                            rel_err(res["m"], one.optimStateG["m"].numpy())]))
    same = []
    for key in ("pG", "m"):
        t = torch.from_numpy(res[key]).clone()
        dist.broadcast(t, 0)
        same.append(bool(torch.equal(t, torch.from_numpy(res[key]))))
    flag = torch.tensor([1.0 if (all(same) and all(checks)) else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        np.save(os.path.join(out_dir, "same.npy"), flag.numpy())
    if not all(checks):
        sys.stderr.write("rank %d checks %s\n" % (rank, checks))
    dist.destroy_process_group()


@pytest.mark.parametrize("mode,world", [("rows", 2), ("rows", 3), ("rows", 4), ("gathered", 2)])
def test_data_parallel_fused_update_by_rows_equals_big_batch(mode, world, tmp_path):
    """VERDICT r4 item 5 on the CPU: the row-sharded fused update with its deferred row exchange (2, 3 — ragged — and 4 gloo ranks) and
    the gathered form walk the single-device big batch's trajectory; replicas (parameters and, after gather_adam_state, Adam's first
    moment) hold the same bits on every rank."""
    mp.spawn(_dp_rows_worker, args=(world, _dp_port(20 + world + (5 if mode == "gathered" else 0)), mode, str(tmp_path)), nprocs=world, join=True)
    pG, pD, m = np.load(str(tmp_path / "ok.npy"))
    assert float(np.load(str(tmp_path / "same.npy"))[0]) == 1.0, "a host-logic check failed or replicas diverged across ranks (see stderr)"
    assert pG < 5e-3 and pD < 5e-3 and m < 5e-3, (pG, pD, m)


_DP_KINDS = ["center", "vid", "center_pipe", "vid_pipe"]


def _dp_port(i):
    return 29500 + (os.getpid() % 2000) + 7 * i


@pytest.mark.parametrize("kind", _DP_KINDS)
def test_data_parallel_world2_equals_big_batch(kind, tmp_path):
    mp.spawn(_dp_worker, args=(2, _dp_port(_DP_KINDS.index(kind)), kind, str(tmp_path)), nprocs=2, join=True)
    pG, pD, gG, rm = np.load(str(tmp_path / "ok.npy"))
    assert float(np.load(str(tmp_path / "same.npy"))[0]) == 1.0, "replicas diverged across ranks"
    # sharded gradients are mean-reduced in a different order than the big batch sums: fp32 tolerance
    assert gG < 5e-5 and rm < 1e-5, (gG, rm)
    assert pG < 5e-3 and pD < 5e-3, (pG, pD)     # Adam amplifies rounding on near-zero gradients


@pytest.mark.parametrize("kind,world", [("center_shard", 2), ("vid_shard", 4)])
def test_data_parallel_with_sharded_adam_equals_big_batch(kind, world, tmp_path):
    """shard_adam: G's gradient is reduce-scattered, every rank updates 1 / world of the parameters with an Adam state of that
    size, the shards are all-gathered — the big batch's trajectory (every element is updated by exactly one rank from the same
    mean gradient), replicas bit-identical."""
    mp.spawn(_dp_worker, args=(world, _dp_port(13 + ["center_shard", "vid_shard"].index(kind)), kind, str(tmp_path)), nprocs=world, join=True)
    pG, pD, gG, rm = np.load(str(tmp_path / "ok.npy"))
    assert float(np.load(str(tmp_path / "same.npy"))[0]) == 1.0, "replicas diverged across ranks"
    assert rm < 1e-5 and pG < 5e-3 and pD < 5e-3, (pG, pD, rm)


@pytest.mark.parametrize("kind", ["center", "vid_pipe"])
def test_data_parallel_world4_equals_big_batch(kind, tmp_path):
    """four ranks, two samples each, SyncBN: the big batch of 8 (the 8-GPU configuration's control flow at half width)"""
    mp.spawn(_dp_worker, args=(4, _dp_port(5 + ["center", "vid_pipe"].index(kind)), kind, str(tmp_path)), nprocs=4, join=True)
    pG, pD, gG, rm = np.load(str(tmp_path / "ok.npy"))
    assert float(np.load(str(tmp_path / "same.npy"))[0]) == 1.0, "replicas diverged across ranks"
    assert gG < 5e-5 and rm < 1e-5, (gG, rm)
    assert pG < 5e-3 and pD < 5e-3, (pG, pD)


@pytest.mark.parametrize("kind,world", [("center_local", 2), ("vid_local", 2), ("center_local", 4)])
def test_data_parallel_with_local_batchnorm_is_the_mean_of_the_shard_gradients(kind, world, tmp_path):
    """sync_bn=False (bench.py's default for N > 1, a documented deviation from the big batch: DESIGN.md): BatchNorm sees the
    rank's shard only, so the result is NOT the big batch's — it is exactly the average over ranks of the single-device
    closures run on each shard, with the replicas' parameters still bit-identical and each rank's running statistics
    those of its own shard."""
    i = 8 + ["center_local", "vid_local"].index(kind) + (2 if world == 4 else 0)
    mp.spawn(_dp_worker, args=(world, _dp_port(i), kind, str(tmp_path)), nprocs=world, join=True)
    _, gD, gG, rm = np.load(str(tmp_path / "ok.npy"))
    assert float(np.load(str(tmp_path / "same.npy"))[0]) == 1.0, "replicas diverged across ranks"
    assert gD < 5e-6 and gG < 5e-5 and rm < 1e-6, (gD, gG, rm)


# ------------------------------------------------------------------ collective bring-up of the C-ABI exchange (backend.bring_up_comm)
class _FakeCommLib:
    def __init__(self, avail):
        self._avail = avail

    def vf_comm_available(self):
        return 0 if self._avail else 2


class _FakeCommBackend:
    """what bring_up_comm touches of a backend, without a GPU: `fail` names the stage this rank fails at"""

    def __init__(self, fail):
        self.lib = _FakeCommLib(fail != "avail")
        self.fail, self.comm, self.destroyed = fail, None, 0

    def comm_unique_id(self):
        return bytes(range(128))

    def init_comm(self, world, rank, cid):
        assert cid == bytes(range(128))
        if self.fail == "init":
            raise RuntimeError("ncclCommInitRank failed (injected)")
        self.comm = object()

    def destroy_comm(self):
        if self.comm is not None:
            self.destroyed += 1
        self.comm = None


def _bringup_worker(rank, world, port, fail_rank, stage, out_dir):
    import json
    import video_filler_amd.backend as vb
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.pop("TORCHELASTIC_USE_AGENT_STORE", None)
    b = _FakeCommBackend(stage if rank == fail_rank else None)
    real_verify = vb.verify_comm
    vb.verify_comm = lambda backend, w, r, n=4096: not (stage == "verify" and r == fail_rank)
    try:
        ok, store = vb.bring_up_comm(b, world, rank)
    finally:
        vb.verify_comm = real_verify
    with open(os.path.join(out_dir, "r%d.json" % rank), "w") as fh:
        json.dump(dict(ok=ok, has_comm=b.comm is not None, destroyed=b.destroyed), fh)
    # rank 0 hosts the store: it stays until every rank has written its file
    import time
    store.add("bye", 1)                  # (a rank's last use of the store)
    while rank == 0 and store.add("bye", 0) < world:
        time.sleep(0.02)


@pytest.mark.parametrize("stage", [None, "avail", "init", "verify"])
def test_comm_bring_up_is_decided_by_all_ranks_together(stage, tmp_path):
    """a per-rank fallback can leave some ranks on vf_comm_* and others in torch.distributed, which hangs.  With
    bring_up_comm a failure on ONE rank — RCCL not loadable, vf_comm_init raising, the start-up self-check of the collectives
    failing — puts EVERY rank on the fallback, and no rank keeps a communicator; with no failure every rank keeps one."""
    import json
    world = 3
    port = _dp_port(17 + [None, "avail", "init", "verify"].index(stage))
    mp.spawn(_bringup_worker, args=(world, port, 1, stage, str(tmp_path)), nprocs=world, join=True)
    res = [json.load(open(os.path.join(str(tmp_path), "r%d.json" % r))) for r in range(world)]
    assert all(r["ok"] == (stage is None) for r in res), res
    assert all(r["has_comm"] == (stage is None) for r in res), res
    if stage == "verify":
        assert all(r["destroyed"] == 1 for r in res)       # everyone had one, everyone dropped it


_AGENT_WORKER = """
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import video_filler_amd.backend as vb
from test_host_logic import _FakeCommBackend
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
stage = os.environ.get("STAGE") or None
b = _FakeCommBackend(stage if rank == 1 else None)
vb.verify_comm = lambda backend, w, r, n=4096: True
ok, store = vb.bring_up_comm(b, world, rank)
open(os.path.join(os.environ["OUT_DIR"], "r" + str(rank) + ".txt"), "w").write(" ".join(str(v) for v in (rank, int(ok), int(b.comm is not None), os.environ.get("TORCHELASTIC_USE_AGENT_STORE"))))
"""


@pytest.mark.parametrize("stage", ["", "init"])
def test_comm_bring_up_under_torchrun_agent_store(stage, tmp_path):
    """the way the driver launches bench.py for N > 1 (`python -m torch.distributed.run ... --master-addr 127.0.0.1`): the launcher's
    agent serves the TCP store and every rank is a client of it (TORCHELASTIC_USE_AGENT_STORE) — the ranks must still agree"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w = tmp_path / "w.py"
    w.write_text(_AGENT_WORKER % (root, os.path.join(root, "tests")))
    env = dict(os.environ, STAGE=stage, OUT_DIR=str(tmp_path))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                          "--master-port", str(_dp_port(23 + (1 if stage else 0))), str(w)], env=env, capture_output=True, text=True, timeout=300)
    files = [tmp_path / ("r%d.txt" % r) for r in range(3)]
    assert all(f.exists() for f in files), out.stdout + out.stderr
    rows = [f.read_text().split() for f in files]      # (one file per rank: concurrent prints interleave)
    want = "0" if stage else "1"
    assert all(r[1] == want and r[2] == want and r[3] == "True" for r in rows), rows


def test_weight_planes_follow_the_parameter_version(cpu_backend):
    """with the trainers managing the weight planes, a direct netG.forward after the iteration's last optim.adam
    must not run on planes of the previous weights.  Host logic: every writer of a flat parameter vector bumps its version,
    and a managed Sequential whose planes are older refreshes before it runs."""
    from video_filler_amd import nn, optim
    from video_filler_amd.backend import param_version
    net = nn.Sequential().add(nn.SpatialConvolution(4, 8, 4, 4, 2, 2, 1, 1)).add(nn.LeakyReLU(0.2, True))
    p, g = net.getParameters()
    net.set_weight_planes_managed(True)
    calls = []
    real = net.refresh_weight_planes
    net.refresh_weight_planes = lambda: (calls.append(1), real())[1]
    x = torch.randn(2, 8, 8, 4).permute(0, 3, 1, 2)
    net.forward(x)
    n0 = len(calls)                       # first use: planes never split for this version
    assert n0 == 1
    net.forward(x)
    assert len(calls) == n0               # nothing moved the parameters: no refresh
    v = param_version(p)
    optim.adam_update(p, g, {"learningRate": 1e-3})
    assert param_version(p) == v + 1
    net.forward(x)
    assert len(calls) == n0 + 1           # the Adam step was seen
    net.load_reference_flat(net.reference_flat().clone())
    net.backward(x, torch.randn(2, 4, 4, 8).permute(0, 3, 1, 2))
    assert len(calls) == n0 + 2           # a checkpoint load too, by the backward walk as well


def test_whole_image_batched_tiles_equal_the_tile_loop(cpu_backend):
    """inference.WholeImageInpainter (all tiles in one batch) against the oracle's tile-by-tile restatement of
    test_vid_wholeim.lua:150-226, both on the CPU: the batching, the vflip rule and the masked paste."""
    from video_filler_amd.inference import WholeImageInpainter
    from video_filler_amd.trainers import build_netG
    from oracle import oracle as O
    rng = np.random.default_rng(4)
    predLen, inputLen, nc, fs, H, W = 4, 2, 3, 128, 128, 512
    ref = O.build_netG(6, 6, 8, 8, 16, True)
    O.weights_init(ref, rng)
    pref, _ = ref.getParameters()
    net = build_netG(6, 6, 8, 8, 16, True)
    net.getParameters()
    net.load_reference_flat(torch.from_numpy(pref.copy()))
    ref.evaluate()
    full = rng.uniform(-1, 1, (predLen * nc, H, W)).astype(np.float32)
    padmask = np.zeros((nc, H, W), np.uint8)
    padmask[:, 30:100, 200:330] = 1
    want_out, want_inp, _ = O.whole_image_inpaint(ref, full, padmask, predLen, inputLen, fs, nc)
    out, inp, _ = WholeImageInpainter(net, predLen, inputLen, fs, nc)(torch.from_numpy(full), torch.from_numpy(padmask))
    assert rel_err(out.numpy(), want_out) < 1e-5 and rel_err(inp.numpy(), want_inp) < 1e-5


def test_center_prepare_and_clip_batcher_on_cpu(cpu_backend):
    from video_filler_amd import data
    from oracle import oracle as O
    rng = np.random.default_rng(8)
    batch = O.synth_center_batch(2, rng)
    ctx, center = data.center_prepare(torch.from_numpy(batch), 4)
    wc, wr = O.center_prepare(batch, 4)
    np.testing.assert_array_equal(ctx.numpy(), wc)
    np.testing.assert_array_equal(center.numpy(), wr)
    cb = data.ClipBatcher(2, 6, 128, rng=np.random.default_rng(1))
    mask = np.zeros((1, 160, 160), np.uint8)
    mask[:, 50:110, 50:110] = 1
    while cb.n < 2:
        cb.add(rng.uniform(0.3, 1, (6, 160, 160)).astype(np.float32), mask)
    c, f, m = cb.batch()
    assert tuple(c.shape) == (2, 6, 128, 128) and float(m.max()) == 1.0
    sel = m.numpy() == 1
    np.testing.assert_array_equal(c.numpy()[sel], np.float32(110.0 / 255.0) * np.float32(2) + np.float32(-1))   # FloatTensor arithmetic: fill, then mul(2):add(-1)
    np.testing.assert_array_equal(c.numpy()[~sel], f.numpy()[~sel])


def test_counter_summary_keys_kernels_the_way_the_bench_line_names_them():
    """bench.py copies `roofline.traffic` from profiles/r*_pmc_bench_traffic*.json by the name its kernel table gives the dominant kernel
    (the library's VF_LAUNCH_TIMED label); scripts/pmc_bench_traffic.py has to derive that same label from the symbol rocprofv3 reports.
    A kernel without a rule falls through to a generic name and the committed bench line silently carries `traffic: null` (round 5's
    first evidence visit, for the patch-fed kernels): pin every symbol a configs[1] / [2] / [4] line has chosen so far, and that the
    labels still exist in the sources."""
    import importlib.util
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pmc_bench_traffic", os.path.join(root, "scripts", "pmc_bench_traffic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = {
        "void k_pconv_patch_g<0, false, false>(PGemm)": "pconv_patchg_128x64_t16_m0",
        "void k_pconv_patch_g<1, false, false>(PGemm)": "pconv_patchg_128x64_t16_m1",
        "void k_pconv_patch_g<2, false, true>(PGemm)": "pconv_patchg_128x64_t4_m2",
        "void k_pconv_patch_g<0, false>(PGemm)": "pconv_patchg_128x64_t16_m0",
        "void k_pconv_patch_g<1, false>(PGemm)": "pconv_patchg_128x64_t16_m1",
        "void k_pconv_patch_g<2, true>(PGemm)": "pconv_patchg_128x64_t4_m2",
        "void k_pconv_patch_tr<4>(PGemm)": "pconv_patch_128x64_t4_c4",
        "void k_pconv_patch_tr<2>(PGemm)": "pconv_patch_128x64_t4_c2",
        "void k_pconv_dma<128, 64, 4, 1, 3>(PGemm)": "pconv_dma_128x64x64_t4_1stage",
        "void k_pconv_dma<128, 64, 16, 2, 3>(PGemm)": "pconv_dma_128x64x64_t16",
        "void k_pconv_dma<128, 64, 4, 2, 1>(PGemm)": "pconv_dma_128x64x64_t4_bf16",
        "void k_igemm<64, 64, 32, 32, true, 2, 3, false, true>(IGemm)": "igemm_64x64_kmajorB_v2_bf16x3_db",
        "void k_igemm<64, 64, 32, 32, false, 2, 3, false, true>(IGemm)": "igemm_64x64_rowB_v2_bf16x3_db",
        "void k_pwgrad_group<1, 3>(VfPWGradGroup)": "pwgrad_group_128x128x32",
        "void k_pwgrad_group<1, 3, 1>(VfPWGradGroup)": "pwgrad_group_128x128x32",
        "void k_pwgrad_group<1, 1, 2>(VfPWGradGroup)": "pwgrad_group_128x128x32_bf16",
        "void k_pwgrad_group<1>(VfPWGradGroup)": "pwgrad_group_128x128x32",
        "void k_pwgrad_group<3, 1>(VfPWGradGroup)": "pwgrad_group_128x128x32",
        "void k_pwgrad_group<1, 2>(VfPWGradGroup)": "pwgrad_group_128x128x32_bf16",
        "void k_pconv<128, 64, 64, 32, 4, 32, false>(PGemm)": "pconv_128x64x32_t4",
        "void k_pconv<128, 64, 64, 32, 4, 32>(PGemm)": "pconv_128x64x32_t4",
        "void k_adam<false>(float*, float const*, float*, float*, long, float, float, float, float, float, int const*)": "adam",
        "void k_adam(float*, float const*, float*, float*, long, float, float, float, float, float, int const*)": "adam",
        "void (anonymous namespace)::k_adam_fused_multi<4, 3>((anonymous namespace)::VfFusedTable)": "adam_fused_wgrad",
        "void (anonymous namespace)::k_conv_thin_in<3>(float const*, float const*)": "conv_thin_in_planes",
    }
    for sym, name in want.items():
        assert mod.bench_name(sym) == name, (sym, mod.bench_name(sym))
    src = "".join(open(os.path.join(root, "video-filler_amd", "csrc", f)).read()
                  for f in os.listdir(os.path.join(root, "video-filler_amd", "csrc")) if f.endswith(".hip"))
    for stem in ("pconv_patchg_128x64_t16_m%d", "pconv_patchg_128x64_t4_m%d", "pconv_patch_128x64_t4_c%d", "pconv_dma_%dx%dx64_%s",
                 "adam_fused_wgrad", "pwgrad_group_128x128x32", "conv_thin_in_planes"):
        assert stem in src, stem
    # every committed summary of this round keys its planes kernels by such labels, not by the fall-through (`pconv_patch_g`)
    import glob
    import json
    for f in glob.glob(os.path.join(root, "profiles", "r05_pmc_bench_traffic*.json")):
        keys = json.load(open(f))["kernels"].keys()
        assert not any(re.fullmatch(r"pconv_patch_(g|h|tr)|pwgrad_group", k) for k in keys), (f, sorted(keys))
