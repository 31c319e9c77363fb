"""Deterministic training and bit-for-bit resume on the MI355X: the gather-form DCN adjoint
(``sgv3d_deform_im2col3x3_backward_det``) against float64, deterministic mode of the small model, checkpoint -> new process ->
resume equal to the uninterrupted run (eager and graphed), and torch AdamW state loaded into the fused update.

Run as ``python tests/test_train_resume_gpu.py child '<json>'`` this file is the child program of the resume tests."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ the deterministic adjoint
def _dx_ref(x, off, dcol, groups):
    """float64 autograd of the oracle's deform_im2col3x3 -> d x, NHWC (on the device)"""
    from oracle import torch_model as TM
    B, H, W, C = x.shape
    xr = nchw(x).to(DEV, torch.float64).requires_grad_(True)
    col = TM.deform_im2col3x3(xr, nchw(off[..., :18]).to(DEV, torch.float64))
    d = dcol.to(DEV, torch.float64).reshape(B, H, W, groups, 9, C // groups).permute(0, 3, 5, 4, 1, 2).reshape(B, C, 9, H, W)
    col.backward(d)
    return nhwc(xr.grad)


def _launch(x, off, dcol, groups, det=True):
    from sgv3d_amd import _lib
    lib = _lib.load()
    B, H, W, C = (int(v) for v in x.shape)
    dx = torch.full_like(x, float("nan"))
    doff = torch.zeros(B, H, W, 18, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    if det:
        nws = lib.sgv3d_deform_im2col3x3_backward_det_workspace_bytes(B, H, W)
        ws = torch.full((nws,), 0xAB, dtype=torch.uint8, device=DEV)
        rc = lib.sgv3d_deform_im2col3x3_backward_det(B, H, W, C, groups, x.data_ptr(), off.data_ptr(), 18, dcol.data_ptr(), dx.data_ptr(),
                                                     doff.data_ptr(), 18, ws.data_ptr(), nws, st)
    else:
        rc = lib.sgv3d_deform_im2col3x3_backward(B, H, W, C, groups, x.data_ptr(), off.data_ptr(), 18, dcol.data_ptr(), dx.data_ptr(),
                                                 doff.data_ptr(), 18, st)
    _lib.check(rc, "deform_im2col3x3_backward")
    torch.cuda.synchronize()
    return dx, doff


def _offsets(kind, B, H, W, g):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    off = torch.empty(B, H, W, 18)
    if kind == "uniform":
        return torch.round((torch.rand(B, H, W, 18, generator=g) * 6 - 3) * 2 ** 16) / 2 ** 16
    if kind == "eighths":
        return torch.randint(-24, 25, (B, H, W, 18), generator=g).float() / 8
    if kind == "int":
        return torch.randint(-2, 3, (B, H, W, 18), generator=g).float()
    for t in range(9):
        if kind == "edge":            # on the border rows / columns, just inside or outside, or far out
            choice = torch.tensor([-1.0, -1.0 + 2 ** -10, 0.0, H - 1.0, H - 2 ** -10, float(H), -40.0])
            th = choice[torch.randint(0, 7, (B, H, W), generator=g)]
            choice_w = torch.tensor([-1.0, -1.0 + 2 ** -10, 0.0, W - 1.0, W - 2 ** -10, float(W), 40.0])
            tw = choice_w[torch.randint(0, 7, (B, H, W), generator=g)]
        elif kind == "collapsed":     # every sample of every image on one pixel
            th, tw = torch.full((B, H, W), H // 2 + 0.25), torch.full((B, H, W), W // 3 + 0.5)
        else:
            raise ValueError(kind)
        off[..., 2 * t] = th - (ys - 1 + t // 3)
        off[..., 2 * t + 1] = tw - (xs - 1 + t % 3)
    return off


CASES = [  # (B, H, W, C, groups, offsets, exact data)
    (2, 5, 7, 4, 1, "eighths", True), (1, 6, 5, 8, 2, "int", True), (2, 4, 6, 16, 4, "uniform", False),
    (1, 6, 7, 64, 4, "uniform", False), (2, 5, 6, 68, 1, "uniform", False), (1, 5, 4, 512, 4, "uniform", False),
    (2, 1, 7, 64, 4, "edge", False), (2, 6, 9, 132, 1, "edge", False), (1, 1, 1, 8, 2, "edge", False),
    (2, 5, 6, 64, 4, "collapsed", True), (1, 7, 8, 1040, 4, "collapsed", True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:5]) + "-" + c[5])
def test_det_adjoint_against_float64(case):
    """d x of the gather form against float64 (relative L2 <= 1e-6; integer data on offsets of 1/8 / 1/4: bitwise); three
    launches give identical bytes; d offset is the atomic path's bitwise; d x of the atomic path agrees within 1e-5."""
    B, H, W, C, groups, kind, exact = case
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W + C + len(kind))
    off = _offsets(kind, B, H, W, g)
    if exact:
        x = torch.randint(-4, 5, (B, H, W, C), generator=g).float()
        dcol = torch.randint(-4, 5, (B, H, W, 9 * C), generator=g).float()
    else:
        x = torch.randn(B, H, W, C, generator=g)
        dcol = torch.randn(B, H, W, 9 * C, generator=g)
    x, off, dcol = x.to(DEV), off.to(DEV), dcol.to(DEV)
    ref = _dx_ref(x, off, dcol, groups)
    runs = [_launch(x, off, dcol, groups) for _ in range(3)]
    dx, doff = runs[0]
    assert bool(torch.isfinite(dx).all())
    for dx2, doff2 in runs[1:]:
        assert torch.equal(dx2.view(torch.int32), dx.view(torch.int32)) and torch.equal(doff2, doff)
    rel = float((dx.double() - ref).norm() / ref.norm().clamp_min(1e-300))
    if exact:
        assert torch.equal(dx.double(), ref), rel
    assert rel <= 1e-6, rel
    dxa, doffa = _launch(x, off, dcol, groups, det=False)
    assert torch.equal(doffa, doff)
    assert float((dxa - dx).norm() / dx.norm().clamp_min(1e-30)) <= 1e-5


def test_det_adjoint_cfg2_layer():
    """the cfg-2 DCN at batch 2: 512 channels at 54 x 96, 4 groups"""
    g = torch.Generator().manual_seed(54)
    B, H, W, C, groups = 2, 54, 96, 512, 4
    off = _offsets("uniform", B, H, W, g).to(DEV)
    x = torch.randn(B, H, W, C, generator=g).to(DEV)
    dcol = torch.randn(B, H, W, 9 * C, generator=g).to(DEV)
    dx, doff = _launch(x, off, dcol, groups)
    dx2, doff2 = _launch(x, off, dcol, groups)
    assert torch.equal(dx2.view(torch.int32), dx.view(torch.int32)) and torch.equal(doff2, doff)
    ref = _dx_ref(x, off, dcol, groups)
    rel = float((dx.double() - ref).norm() / ref.norm())
    assert rel <= 1e-6, rel
    dxa, _ = _launch(x, off, dcol, groups, det=False)
    assert float((dxa - dx).norm() / dx.norm()) <= 1e-5


def test_det_adjoint_rejects_before_launch():
    from sgv3d_amd import _lib
    lib = _lib.load()
    B, H, W, C = 1, 4, 4, 16
    x = torch.randn(B, H, W, C, device=DEV)
    off = torch.zeros(B, H, W, 18, device=DEV)
    dcol = torch.randn(B, H, W, 9 * C, device=DEV)
    dx = torch.full((B, H, W, C), 9.0, device=DEV)
    doff = torch.full((B, H, W, 18), 9.0, device=DEV)
    nws = lib.sgv3d_deform_im2col3x3_backward_det_workspace_bytes(B, H, W)
    assert nws > 0 and lib.sgv3d_deform_im2col3x3_backward_det_workspace_bytes(0, H, W) == 0
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    f = lib.sgv3d_deform_im2col3x3_backward_det
    bad = [
        lambda: f(B, H, W, 8, 4, P(x), P(off), 18, P(dcol), P(dx), P(doff), 18, P(ws), nws, st),          # 8 % 16
        lambda: f(B, H, W, C, 4, P(x), P(off), 17, P(dcol), P(dx), P(doff), 18, P(ws), nws, st),
        lambda: f(B, H, W, C, 4, P(x), P(off), 18, P(dcol), P(dx), P(doff), 18, None, nws, st),
        lambda: f(B, H, W, C, 4, P(x), P(off), 18, P(dcol), P(dx), P(doff), 18, P(ws), nws - 4, st),
        lambda: f(B, H, W, C, 4, P(x), P(off), 18, P(dcol) + 4, P(dx), P(doff), 18, P(ws), nws, st),      # misaligned
    ]
    for call in bad:
        assert call() != 0
    torch.cuda.synchronize()
    assert bool((dx == 9.0).all()) and bool((doff == 9.0).all())


# ------------------------------------------------------------------------------------------------ the small model, deterministic
def _setup(bucket_bytes=None):
    from sgv3d_amd import synthetic
    from sgv3d_amd.models.bev_height import BEVHeight
    from sgv3d_amd.train_step import DataParallelAdamW
    dev = torch.device(DEV)
    bconf, hconf = synthetic.small_conf()
    torch.manual_seed(0)
    torch.cuda.manual_seed_all(0)
    model = BEVHeight(bconf, hconf).to(dev).train()          # (ASPP dropout 0.5 active: the random stream is part of the state)
    model.head.train_cfg = dict(model.head.train_cfg, grid_size=[256, 256, 1], point_cloud_range=[0, -12.8, -5, 25.6, 12.8, 3])
    imgs = synthetic.make_images(2, final=bconf['final_dim'], device=dev, seed=0)
    mats = synthetic.make_mats(2, device=dev, scale=bconf['final_dim'][0] / 864)
    boxes, labels = synthetic.make_gt(2, seed=0, n_range=(10, 40), stress=False)
    boxes, labels = [b.to(dev) for b in boxes], [l.to(dev) for l in labels]
    opt = DataParallelAdamW(model.parameters(), lr=2e-4, max_grad_norm=5.0, bucket_bytes=bucket_bytes)

    def forward_backward():
        loss = model.loss(model.get_targets(boxes, labels), model(imgs, mats))
        loss.backward()
        return loss
    return model, opt, forward_backward


def _state(model, opt, losses):
    return {'params': [p.detach().cpu().clone() for p in model.parameters()],
            'buffers': [b.detach().cpu().clone() for b in model.buffers()],
            'moments': copy.deepcopy({i: {k: v.cpu() for k, v in e.items()} for i, e in opt.state_dict()['state'].items()}),
            'steps': opt.steps, 'losses': losses}


def _equal(a, b):
    assert a['steps'] == b['steps'] and a['losses'] == b['losses'], (a['losses'], b['losses'])
    assert all(torch.equal(x, y) for x, y in zip(a['params'], b['params']))
    assert all(torch.equal(x, y) for x, y in zip(a['buffers'], b['buffers']))
    assert a['moments'].keys() == b['moments'].keys()
    for i in a['moments']:
        assert all(torch.equal(a['moments'][i][k], b['moments'][i][k]) for k in ('exp_avg', 'exp_avg_sq')), i


def test_small_model_deterministic_mode_is_bitwise_repeatable():
    """Two 3-step runs of the small model from one seed under torch.use_deterministic_algorithms(True) (Lightning's
    deterministic=True): bitwise-equal parameters, moments, BatchNorm buffers and losses.  The flag is restored afterwards."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            model, opt, fb = _setup()
            losses = []
            for _ in range(3):
                opt.zero_grad()
                losses.append(float(fb().detach()))
                opt.step()
            runs.append(_state(model, opt, losses))
            del model, opt, fb
    finally:
        torch.use_deterministic_algorithms(was)
    _equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------ resume in a new process
def _child(cfg):
    sys.path.insert(0, ROOT)
    from sgv3d_amd import hip_ops
    from sgv3d_amd.checkpoint import load_checkpoint, save_checkpoint
    from sgv3d_amd.train_step import GraphedTrainStep
    hip_ops.DETERMINISTIC = True
    bucket = cfg.get('bucket_mib')
    model, opt, fb = _setup(None if bucket is None else bucket << 20)
    if cfg.get('load'):
        load_checkpoint(cfg['load'], model, opt)
    if cfg['graph']:
        step = GraphedTrainStep(fb, opt, warmup=2, strict=True, keep_state=model)
    else:
        def step():
            opt.zero_grad()
            loss = fb()
            opt.step()
            return loss
    losses = []
    for i in range(cfg['steps']):
        losses.append(float(step().detach()))
        if cfg.get('save_after') == i + 1:
            torch.cuda.synchronize()
            save_checkpoint(cfg['save'], model, opt, epoch=0, global_step=opt.steps)
    torch.cuda.synchronize()
    torch.save(_state(model, opt, losses), cfg['out'])


def _spawn(cfg):
    env = {k: v for k, v in os.environ.items() if k not in ("SGV3D_FORCE_DIST", "RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), "child", json.dumps(cfg)], env=env, cwd=ROOT,
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _wait(procs):
    for p in procs:
        try:
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
            raise AssertionError("child timed out:\n" + out[-3000:])
        assert p.returncode == 0, out[-3000:]


def test_resume_in_a_new_process_is_bitwise_the_uninterrupted_run(tmp_path):
    """4 steps against 2 steps + checkpoint + a new process + load + 2 steps, eager and as GraphedTrainStep replays
    (keep_state): bitwise-equal parameters, moments, BatchNorm buffers, step counter and losses.  Loaded with a different bucket
    size the run continues within 1e-6 relative (the clip norm's partial sums follow the bucket layout)."""
    t = lambda name: str(tmp_path / name)
    first = [_spawn(dict(graph=g, steps=4, save_after=2, save=t(f"{g}.ckpt"), out=t(f"{g}_full.pt"))) for g in (False, True)]
    _wait(first)
    second = [_spawn(dict(graph=g, steps=2, load=t(f"{g}.ckpt"), out=t(f"{g}_resumed.pt"))) for g in (False, True)]
    second.append(_spawn(dict(graph=False, steps=2, load=t("False.ckpt"), bucket_mib=1, out=t("bucket_resumed.pt"))))
    _wait(second)
    for g in (False, True):
        full = torch.load(t(f"{g}_full.pt"), weights_only=False)
        resumed = torch.load(t(f"{g}_resumed.pt"), weights_only=False)
        full['losses'] = full['losses'][2:]
        _equal(full, resumed)
    full = torch.load(t("False_full.pt"), weights_only=False)
    other = torch.load(t("bucket_resumed.pt"), weights_only=False)
    a, b = torch.cat([p.reshape(-1) for p in full['params']]), torch.cat([p.reshape(-1) for p in other['params']])
    assert float((a - b).norm() / a.norm()) <= 1e-6


# ------------------------------------------------------------------------------------------------ torch AdamW state -> fused step
def test_fused_step_after_loading_torch_adamw_state():
    """torch.optim.AdamW runs 3 steps; its state_dict() loaded into DataParallelAdamW over a copy of the parameters; one more step
    of each on the same gradients agrees to 1e-6."""
    from sgv3d_amd.train_step import DataParallelAdamW
    g = torch.Generator(device=DEV).manual_seed(3)
    shapes = [(64, 32, 3, 3), (64,), (7, 64), (5,)]
    ref = [torch.randn(s, device=DEV, generator=g).requires_grad_(True) for s in shapes]
    ropt = torch.optim.AdamW(ref, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.05)
    for _ in range(3):
        for p in ref:
            p.grad = torch.randn(p.shape, device=DEV, generator=g)
        ropt.step()
    ours = [p.detach().clone().requires_grad_(True) for p in ref]
    opt = DataParallelAdamW(ours, lr=1.0, bucket_bytes=4096)
    opt.load_state_dict(copy.deepcopy(ropt.state_dict()))
    grads = [torch.randn(p.shape, device=DEV, generator=g) for p in ref]
    for p, q, gr in zip(ours, ref, grads):
        p.grad.copy_(gr)
        q.grad = gr.clone()
    opt.step()
    ropt.step()
    for p, q in zip(ours, ref):
        err = float((p.detach() - q.detach()).abs().max() / q.detach().abs().max())
        assert err <= 1e-6, err


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "child":
    _child(json.loads(sys.argv[2]))
