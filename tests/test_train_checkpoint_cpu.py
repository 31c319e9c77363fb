"""CPU: DataParallelAdamW's optimiser state in torch.optim.AdamW's layout, and the checkpoint file of sgv3d_amd.checkpoint
(pytorch-lightning 1.5.10 layout: what the reference harness's ModelCheckpoint writes and ``--ckpt_path`` reads)."""
import copy

import pytest
import torch

from sgv3d_amd._lib import SGV3DError
from sgv3d_amd.train_step import DataParallelAdamW


def _module():
    torch.manual_seed(0)
    m = torch.nn.ModuleDict({
        'a': torch.nn.Linear(5, 7),
        'frozen': torch.nn.Linear(7, 3),
        'unused': torch.nn.Linear(4, 4),          # never receives a gradient
        'b': torch.nn.Linear(7, 2, bias=False),
    })
    m['frozen'].weight.requires_grad_(False)
    return m


def _torch_run(steps=3):
    m = _module()
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3, betas=(0.9, 0.99), eps=1e-7, weight_decay=0.05)
    g = torch.Generator().manual_seed(1)
    for _ in range(steps):
        opt.zero_grad()
        x = torch.randn(6, 5, generator=g)
        h = torch.relu(m['a'](x))
        (m['b'](h).square().mean() + m['frozen'](h).square().mean()).backward()
        opt.step()
    return m, opt


def _sd(opt):
    return copy.deepcopy(opt.state_dict())        # (torch's state_dict shares the per-parameter dicts with the optimiser)


def _same(a, b):
    assert a.keys() == b.keys()
    assert a['param_groups'] == b['param_groups']
    assert a['state'].keys() == b['state'].keys()
    for i in a['state']:
        ea, eb = a['state'][i], b['state'][i]
        assert ea.keys() == eb.keys()
        assert float(ea['step']) == float(eb['step'])
        for k in ('exp_avg', 'exp_avg_sq'):
            assert ea[k].dtype == eb[k].dtype and torch.equal(ea[k], eb[k]), (i, k)


@pytest.mark.parametrize("bucket_bytes", [64, 48 << 20])
def test_torch_adamw_state_round_trips(bucket_bytes):
    """torch's AdamW state (frozen parameter and never-used parameter without state) loaded into DataParallelAdamW over the
    same parameters comes back from state_dict() equal: keys, indices, hyperparameters, bitwise moments."""
    m, ref = _torch_run()
    want = ref.state_dict()
    assert set(want['state']) == {0, 1, 3, 6}              # frozen.weight (2) and unused.* (4, 5) carry no state
    ours = DataParallelAdamW(m.parameters(), lr=1.0, bucket_bytes=bucket_bytes)
    ours.load_state_dict(want)
    assert ours.steps == 3 and ours.lr == 2e-3 and ours.betas == (0.9, 0.99) and ours.eps == 1e-7 and ours.weight_decay == 0.05
    _same(ours.state_dict(), want)


def test_step_as_int_of_torch_1_9():
    m, ref = _torch_run()
    sd = _sd(ref)
    for e in sd['state'].values():
        e['step'] = int(e['step'])
    ours = DataParallelAdamW(m.parameters(), lr=1.0)
    ours.load_state_dict(sd)
    assert ours.steps == 3
    _same(ours.state_dict(), ref.state_dict())


def test_fresh_optimiser_has_no_state_and_torch_keys():
    m = _module()
    ours = DataParallelAdamW(m.parameters(), lr=2e-3)
    ref = torch.optim.AdamW(m.parameters(), lr=2e-3, weight_decay=1e-7)
    _same(ours.state_dict(), ref.state_dict())


def test_bad_state_raises_and_writes_nothing():
    m, ref = _torch_run()
    ours = DataParallelAdamW(m.parameters(), lr=1.0, bucket_bytes=64)
    ours.load_state_dict(ref.state_dict())
    before = ours.state_dict()

    bad_shape = _sd(ref)
    bad_shape['state'][6]['exp_avg'] = torch.zeros(3, 7)
    with pytest.raises(SGV3DError, match="parameter 6"):
        ours.load_state_dict(bad_shape)
    bad_steps = _sd(ref)
    bad_steps['state'][1]['step'] = torch.tensor(2.0)
    with pytest.raises(SGV3DError, match="different step counts"):
        ours.load_state_dict(bad_steps)
    bad_count = _sd(ref)
    bad_count['param_groups'][0]['params'] = bad_count['param_groups'][0]['params'][:-1]
    with pytest.raises(SGV3DError, match="parameters"):
        ours.load_state_dict(bad_count)
    frozen = _sd(ref)
    frozen['state'][2] = dict(frozen['state'][0], exp_avg=torch.zeros(3, 7), exp_avg_sq=torch.zeros(3, 7))
    with pytest.raises(SGV3DError, match="does not train"):
        ours.load_state_dict(frozen)
    _same(ours.state_dict(), before)
    assert ours.steps == 3


def test_missing_entries_get_zero_moments():
    m, ref = _torch_run()
    sd = _sd(ref)
    del sd['state'][1]
    ours = DataParallelAdamW(m.parameters(), lr=1.0, bucket_bytes=64)
    ours.load_state_dict(ref.state_dict())
    ours.load_state_dict(sd)
    got = ours.state_dict()
    assert set(got['state']) == {0, 3, 6}
    bi, off, cnt = ours.flat.where[id(m['a'].bias)]
    assert not ours.state[bi][0][off:off + cnt].any() and not ours.state[bi][1][off:off + cnt].any()


def test_checkpoint_file_layout_and_strict_reload(tmp_path):
    """save_checkpoint of a CPU-built BEVHeight: Lightning 1.5.10 keys, 'model.'-prefixed state_dict, AdamW state,
    MultiStepLR state; the stripped state_dict loads strictly into a fresh model with bitwise-equal tensors."""
    from sgv3d_amd import synthetic
    from sgv3d_amd.checkpoint import load_checkpoint, save_checkpoint
    from sgv3d_amd.models.bev_height import BEVHeight
    bconf, hconf = synthetic.small_conf()
    torch.manual_seed(0)
    model = BEVHeight(bconf, hconf)
    synthetic.randomize_norm_stats_(model, 1)
    opt = DataParallelAdamW(model.parameters(), lr=2e-4)
    path = str(tmp_path / "epoch=4.ckpt")
    save_checkpoint(path, model, opt, epoch=20, global_step=1234, extra={'sampler_epoch': 20})
    ck = torch.load(path, map_location='cpu', weights_only=False)
    for k in ('epoch', 'global_step', 'pytorch-lightning_version', 'state_dict', 'optimizer_states', 'lr_schedulers', 'sgv3d'):
        assert k in ck, k
    assert (ck['epoch'], ck['global_step'], ck['pytorch-lightning_version']) == (20, 1234, "1.5.10")
    names = list(model.state_dict())
    assert list(ck['state_dict']) == ['model.' + n for n in names]
    assert len(ck['optimizer_states']) == 1
    assert ck['optimizer_states'][0]['param_groups'][0]['params'] == list(range(len(list(model.parameters()))))
    sched = ck['lr_schedulers'][0]
    assert sched['last_epoch'] == 20 and dict(sched['milestones']) == {19: 1, 23: 1} and sched['gamma'] == 0.1
    assert sched['_last_lr'] == [pytest.approx(2e-5)]
    assert ck['sgv3d']['format_version'] == 1 and ck['sgv3d']['extra'] == {'sampler_epoch': 20}

    torch.manual_seed(1)
    fresh = BEVHeight(bconf, hconf)
    fresh.load_state_dict({k[len('model.'):]: v for k, v in ck['state_dict'].items()}, strict=True)
    for (n, a), (_, b) in zip(model.state_dict().items(), fresh.state_dict().items()):
        assert torch.equal(a, b), n

    torch.manual_seed(2)
    other = BEVHeight(bconf, hconf)
    meta = load_checkpoint(path, other)
    assert meta['epoch'] == 20 and meta['global_step'] == 1234 and meta['extra'] == {'sampler_epoch': 20}
    for (n, a), (_, b) in zip(model.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), n
