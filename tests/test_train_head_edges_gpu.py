"""CenterHead target assignment and loss on the MI355X through the C ABI, at the shapes the head's one configuration never
reaches: non-square maps, more than 64 boxes, windows cut on every side, unaligned outputs, the slot split of the box kernel,
the clamp bounds, injected averaging factors, gradient scale and batch strides.  References: the oracle for the targets,
float64 torch autograd (and the oracle) for the loss; the bars are those of test_train_head_gpu.py."""
import numpy as np
import pytest
import torch

import train_head_abi as A
from oracle import train_head_ref as R

pytestmark = pytest.mark.gpu

MAPS = ('heat',) + tuple(k for k, _ in A.BRANCHES)
_RUNS = {}


def run(name):
    """(case, kernel outputs, oracle outputs) of a target case, computed once."""
    if name not in _RUNS:
        case = A.TARGET_CASES[name]()
        _RUNS[name] = (case, A.targets(**case), A.oracle_targets(**case))
    return _RUNS[name]


def check_targets(got, want):
    assert got['rc'] == 0
    assert np.array_equal(got['ind'], want['ind']), "ind"
    assert np.array_equal(got['mask'], want['mask']), "mask"
    np.testing.assert_allclose(got['anno'], want['anno'], rtol=2e-6, atol=2e-7, err_msg="anno_box")
    assert np.array_equal(got['heatmap'] == 1.0, want['heatmap'] == 1.0), "peaks"
    assert np.array_equal(got['heatmap'] == 0.0, want['heatmap'] == 0.0), "support of the Gaussians"
    assert np.abs(got['heatmap'] - want['heatmap']).max() <= 6e-8


# ------------------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize("name", ['nonsquare_24x40', 'nonsquare_40x24'])
def test_targets_nonsquare(name):
    case, got, want = run(name)
    check_targets(got, want)
    assert got['mask'][:, 1].sum() == 0 and (got['heatmap'][1] == 0).all()          # the sample without boxes


@pytest.fixture(scope="module")
def head():
    from sgv3d_amd import synthetic
    from sgv3d_amd.layers.heads.bev_height_head import BEVHeightHead
    _, conf = synthetic.r50_256_conf()
    conf['tasks'] = [dict(num_class=1, class_names=['a']), dict(num_class=3, class_names=['b', 'c', 'd'])]
    return BEVHeightHead(**conf).cuda().eval()


def _module_targets(head, case):
    cfg = A.train_cfg(case['max_objs'], case['h'], case['w'], case['pc'])
    boxes = [torch.from_numpy(case['boxes'][0]), torch.zeros(0, 9)]
    labels = [torch.from_numpy(case['labels'][0]).long(), torch.zeros(0, dtype=torch.long)]
    old = head.train_cfg
    head.train_cfg = cfg
    try:
        got = head.get_targets([b.cuda() for b in boxes], [l.cuda() for l in labels])
    finally:
        head.train_cfg = old
    return cfg, got


@pytest.mark.parametrize("name", ['nonsquare_24x40', 'nonsquare_40x24'])
def test_nonsquare_through_the_module(head, name):
    case, _, want = run(name)
    h, w = case['h'], case['w']
    cfg, tg = _module_targets(head, case)
    assert tuple(tg[0][1].shape) == (2, 3, h, w)
    got = dict(rc=0, heatmap=torch.cat(tg[0], 1).cpu().numpy(), anno=torch.stack(tg[1]).cpu().numpy(),
               ind=torch.stack(tg[2]).cpu().numpy(), mask=torch.stack(tg[3]).cpu().numpy())
    check_targets(got, want)
    # the loss on these targets against the oracle
    g = torch.Generator().manual_seed(h)
    buf = torch.randn(2, 24, h, w, generator=g).cuda()
    preds, c0 = [], 0
    for nc in (1, 3):
        d = {}
        for k, c in A.BRANCHES + (('heatmap', nc),):
            d[k] = buf[:, c0:c0 + c]
            c0 += c
        preds.append([d])
    old = head.train_cfg
    head.train_cfg = cfg
    try:
        loss = float(head.loss(tg, preds))
    finally:
        head.train_cfg = old
    total, _ = R.loss(tuple([x.cpu().numpy() for x in part] for part in tg),
                      [{k: v.cpu().numpy() for k, v in pl[0].items()} for pl in preds], cfg['code_weights'], 0.25)
    assert abs(loss - total) <= 2e-5 * abs(total)


@pytest.mark.parametrize("n_max", [64, 65, 128, 130, 200])
def test_targets_more_than_64_boxes(n_max):
    case, got, want = run(f'many_{n_max}')
    check_targets(got, want)
    # the slot is the permutation the definition gives: z of the box sits in its slot
    slots = A.expected_slots(case['labels'], case['classes_per_task'])
    cy, cx, inside = A.cells(case)
    for b in range(3):
        for i in np.where((slots[b] >= 0) & inside[b])[0]:
            k = slots[b, i]
            assert got['mask'][0, b, k] == 1 and got['ind'][0, b, k] == cy[b, i] * case['w'] + cx[b, i], (b, i, k)
            assert got['anno'][0, b, k, 2] == case['boxes'][b, i, 2], (b, i, k)
    assert got['mask'].sum() == ((slots >= 0) & inside).sum() > 0.8 * (slots >= 0).sum()


@pytest.mark.parametrize("max_objs", [1, 64, 65])
def test_targets_cut_by_max_objs(max_objs):
    case, got, want = run(f'cut_{max_objs}')
    check_targets(got, want)
    assert got['mask'][0].sum() == max_objs and got['mask'][1].sum() == 0
    assert (got['heatmap'] == 1).sum() <= max_objs                 # boxes past the cut draw nothing


@pytest.mark.parametrize("name", ['edges_5x7', 'edges_1x9', 'edges_1x1'])
def test_targets_windows_against_the_edges(name):
    case, got, want = run(name)
    check_targets(got, want)
    assert got['mask'][0, :, 0].all()
    if name != 'edges_1x9':
        assert (got['heatmap'] > 0).all()                                    # the window covers the whole map


def test_targets_known_answers():
    case, got, _ = run('known')
    K = A.known_answers()
    assert got['rc'] == 0
    assert np.array_equal(got['mask'][0, 0], K['mask']) and np.array_equal(got['ind'][0, 0], K['ind'])
    assert np.array_equal(got['anno'][0, 0, :, :2], K['res'])
    live = K['mask'] == 1
    np.testing.assert_allclose(got['anno'][0, 0][live][:, 2:], np.tile(K['rest'], (4, 1)), rtol=2e-6, atol=2e-7)
    assert (got['anno'][0, 0][~live] == 0).all()                     # a skipped box leaves its slot empty
    assert sorted(map(tuple, np.argwhere(got['heatmap'][0, 0] == 1))) == sorted(K['peaks'])


def test_targets_radius_sweep():
    case, got, want = run('radius_sweep')
    check_targets(got, want)


def test_targets_max_merge():
    case, got, want = run('max_merge')
    check_targets(got, want)
    hm = got['heatmap']
    assert hm[0, 1, 6, 5] == 1 and hm[0, 1, 6, 8] == 1 and (hm[0, 0] == 0).all()
    assert hm[1, 0, 4, 4] == 1 and hm[1, 1, 4, 4] == 1 and (hm[1, 0] > 0).sum() > (hm[1, 1] > 0).sum()


def test_targets_unaligned_outputs():
    case = dict(A.case_nonsquare(24, 40), max_objs=37)                # 148 slots: no multiple of 16
    base = A.targets(**case)
    check_targets(base, A.oracle_targets(**case))
    for shifts in ((4, 12, 8, 3), (12, 4, 24, 1)):
        got = A.targets(**case, shifts=shifts, launches=2)
        assert got['rc'] == 0
        for a, b, c in zip(base['runs'][0], got['runs'][0], got['runs'][1]):
            assert np.array_equal(a, b) and np.array_equal(a, c)


def _tiny(**kw):
    boxes = np.zeros((2, 3, 9), np.float32)
    boxes[:, :, :2], boxes[:, :, 3:6] = 1.0, 1.0
    case = dict(boxes=boxes, labels=np.zeros((2, 3), np.int32), classes_per_task=[1, 2], max_objs=5, h=4, w=6)
    case.update(kw)
    return case


@pytest.mark.parametrize("kw", [
    dict(classes_per_task=[1] * 17), dict(classes_per_task=[33]), dict(classes_per_task=[16, 17]), dict(classes_per_task=[2, 0, 1]),
    dict(max_objs=0), dict(voxel=(0.0, 0.1)), dict(null=('heatmap',)), dict(null=('anno',)), dict(null=('ind',)),
    dict(null=('mask',)), dict(null=('boxes',)), dict(null=('labels',))], ids=str)
def test_targets_rejections(kw):
    got = A.targets(**_tiny(**kw))
    assert got['rc'] != 0 and got['untouched']


def test_targets_without_boxes_zero_everything():
    got = A.targets(None, None, [1, 2], 5, 4, 6, batch=2, n_max=0)
    assert got['rc'] == 0
    assert all((r == 0).all() for r in got['runs'][0])


def test_targets_share_of_differing_cells():
    """The cap of test_train_head_gpu.py on heatmap cells that differ at all, over all target cases pooled."""
    differ = total = 0
    for name in A.TARGET_CASES:
        _, got, want = run(name)
        differ += int((got['heatmap'] != want['heatmap']).sum())
        total += want['heatmap'].size
    print(f"differing heatmap cells: {differ} of {total}")
    assert differ / total < 1e-4


# ---------------------------------------------------------------------------------------------------------------- loss
def ref_loss(inp, stats=None, grad_scale=1.0, code_weights=A.CODE_WEIGHTS, box_weight=0.25):
    """float64 autograd on the CPU.  A slot whose index lies outside the map is dropped from the sum (the kernel's documented
    behaviour) but stays in the mask count, as in ``sgv3d_centerhead_loss_stats``."""
    t = {k: torch.from_numpy(np.asarray(inp[k], np.float64)).requires_grad_(True) for k in MAPS}
    tgt = torch.from_numpy(np.asarray(inp['target'], np.float64))
    B, cat, h, w = tgt.shape
    ind, live = inp['ind'], (inp['mask'] != 0) & (inp['ind'] >= 0) & (inp['ind'] < h * w)
    if stats is None:
        stats = (float((inp['target'] == 1).sum()), float((inp['mask'] != 0).sum()))
    avg, num = max(float(stats[0]), 1.0), max(float(stats[1]), 1e-4)
    heat = torch.clamp(torch.sigmoid(t['heat']), 1e-4, 1 - 1e-4)
    pos = tgt.eq(1).double()
    l_heat = (-(heat + 1e-12).log() * (1 - heat) ** 2 * pos - (1 - heat + 1e-12).log() * heat ** 2 * (1 - tgt) ** 4 * (1 - pos)).sum() / avg
    anno = torch.cat([t[k] for k, _ in A.BRANCHES], 1)
    flat = anno.permute(0, 2, 3, 1).reshape(B, h * w, 10)
    idx = torch.from_numpy(np.where(live, ind, 0))[:, :, None].expand(-1, -1, 10)
    m = torch.from_numpy(live.astype(np.float64))[:, :, None] * torch.tensor(code_weights, dtype=torch.float64)
    l_box = ((flat.gather(1, idx) - torch.from_numpy(np.asarray(inp['anno'], np.float64))).abs() * m).sum() / num * box_weight
    (l_heat + l_box).backward()
    out = dict(loss=(float(l_heat.detach()), float(l_box.detach())))
    for k in MAPS:
        out['g_' + k] = t[k].grad.numpy() * grad_scale
    return out


def check_loss(got, want):
    assert got['rc'] == 0 and got['stats_rc'] == 0
    assert np.isfinite(got['loss']).all()
    for i in range(2):
        assert abs(float(got['loss'][i]) - want['loss'][i]) <= 2e-5 * abs(want['loss'][i]), (i, got['loss'], want['loss'])
    scale = max(float(np.abs(want['g_' + k]).max()) for k in MAPS)
    for k in MAPS:
        assert np.isfinite(got['g_' + k]).all(), k
        assert float(np.abs(got['g_' + k] - want['g_' + k]).max()) <= 2e-5 * scale, k


@pytest.mark.parametrize("cat,batch,max_objs,h,w", [(1, 1, 1, 5, 9), (2, 3, 7, 9, 5), (3, 1, 8, 5, 9), (1, 3, 9, 9, 5),
                                                     (2, 1, 64, 5, 9), (3, 3, 300, 9, 5), (2, 1, 2100, 5, 9)])
def test_loss_shapes(cat, batch, max_objs, h, w):
    inp = A.loss_inputs(100 + max_objs, batch, cat, h, w, max_objs)
    got = A.loss(inp)
    check_loss(got, ref_loss(inp))
    assert np.array_equal(got['stats'], np.array([(inp['target'] == 1).sum(), inp['mask'].sum()], np.float32))
    total, _ = R.loss(([inp['target']], [inp['anno']], [inp['ind']], [inp['mask']]),
                      [dict(heatmap=inp['heat'], **{k: inp[k] for k, _ in A.BRANCHES})], A.CODE_WEIGHTS, 0.25)
    assert abs(float(got['loss'].astype(np.float64).sum()) - total) <= 2e-5 * abs(total)


@pytest.mark.parametrize("max_objs,phase", [(7, 0), (7, 1), (8, 0), (8, 1), (9, 0), (64, 0), (300, 0)])
def test_loss_shared_cells_across_the_split(max_objs, phase):
    inp = A.shared_straddle(max_objs, phase)
    check_loss(A.loss(inp), ref_loss(inp))


@pytest.mark.parametrize("max_objs", [7, 64, 300])
def test_loss_all_slots_on_one_cell(max_objs):
    inp = A.shared_one_cell(max_objs)
    check_loss(A.loss(inp), ref_loss(inp))


def test_loss_shared_cell_more_than_256_slots_apart():
    inp, _, _ = A.shared_far_trio()
    check_loss(A.loss(inp), ref_loss(inp))


@pytest.mark.parametrize("batch,grad_scale", [(1, 1.0), (2, 0.5)])
def test_loss_shared_cell_known_answer(batch, grad_scale):
    inp = A.shared_one_cell(8, batch=batch)
    for k, _ in A.BRANCHES:
        inp[k][:] = 0
    inp['anno'] = np.abs(inp['anno']) + 0.5
    got = A.loss(inp, grad_scale=grad_scale)
    assert got['rc'] == 0
    num = 8 * batch
    for b in range(batch):
        cell = int(inp['ind'][b, 0])
        c0 = 0
        for k, c in A.BRANCHES:
            g = got['g_' + k][b].reshape(c, -1)
            want = np.zeros_like(g)
            want[:, cell] = [np.float32(-8 * A.CODE_WEIGHTS[c0 + j] * 0.25 * grad_scale / num) for j in range(c)]
            assert np.array_equal(g, want), (b, k)
            c0 += c


def test_loss_index_hygiene():
    inp = A.loss_inputs(70, 2, 2, 5, 9, 9, live=1.1)
    big = np.iinfo(np.int64).max
    for (b, k), (m, i) in {(0, 1): (0, -1), (0, 2): (0, 45), (1, 0): (0, big),                     # masked off
                           (1, 3): (1, 45), (0, 4): (1, -1), (1, 5): (1, big), (0, 6): (1, -big - 1)}.items():   # live, outside
        inp['mask'][b, k], inp['ind'][b, k] = m, i
    got = A.loss(inp)
    check_loss(got, ref_loss(inp))
    assert got['stats'][1] == inp['mask'].sum() == 15


def test_loss_clamp():
    inp = A.clamp_inputs()
    got, want = A.loss(inp), ref_loss(inp)
    check_loss(got, want)
    x = np.array(A.CLAMP_LOGITS, np.float64)
    outside = np.abs(x) > A.LN9999
    for row in range(3):
        g = got['g_heat'][0, 0, row]
        assert (g[outside] == 0).all() and (g[~outside & (x != 0)] != 0).all(), row


@pytest.mark.parametrize("x", [9.5, 20.0, 88.0, 100.0, -9.5, -20.0, -88.0, -100.0])
@pytest.mark.parametrize("t", [1.0, 0.0])
def test_loss_of_saturated_cells_is_the_closed_form(x, t):
    """All 45 cells at one saturated logit: the loss is the closed form at the float32 clamp bound p, with q = 1 - p taken at its
    float32 value as well (the rounding of 1 - 1e-4 is 1.7e-4 of the logarithm of a target-0 cell, a property of the format)."""
    inp = A.loss_inputs(61, 1, 1, 5, 9, 2, live=-1.0)
    inp['heat'][:], inp['target'][:] = x, t
    got = A.loss(inp)
    assert got['rc'] == 0 and (got['g_heat'] == 0).all()
    lo, hi = np.float64(np.float32(1e-4)), np.float64(np.float32(1) - np.float32(1e-4))
    p = hi if x > 0 else lo
    q = np.float64(np.float32(1) - np.float32(p))
    cell = -np.log(p + 1e-12) * q ** 2 if t == 1.0 else -np.log(q + 1e-12) * p ** 2
    want = cell if t == 1.0 else 45 * cell                            # 45 positives, or none (the divisor clamps to 1)
    assert abs(float(got['loss'][0]) - want) <= 2e-5 * want, (got['loss'][0], want)
    assert got['loss'][1] == 0


def test_loss_positives_are_cells_of_exactly_one():
    inp = A.loss_inputs(62, 2, 2, 5, 9, 9)
    below = np.nextafter(np.float32(1), np.float32(0))
    inp['target'][:, :, 1, ::2] = below
    inp['target'][:, :, 2, 1::2] = 1.0
    got, want = A.loss(inp), ref_loss(inp)
    assert np.array_equal(got['stats'].astype(np.int64), [int((inp['target'] == 1).sum()), int(inp['mask'].sum())])
    assert (inp['target'] == below).sum() >= 20
    check_loss(got, want)


@pytest.mark.parametrize("stats", [(2.5, 3.5), (0.0, 0.0)])
def test_loss_injected_stats(stats):
    inp = A.loss_inputs(63, 3, 2, 9, 5, 9)
    got = A.loss(inp, stats=stats)
    check_loss(got, ref_loss(inp, stats=stats))
    assert np.array_equal(got['stats'], np.array(stats, np.float32))          # an input: left as it was


def test_loss_grad_scale():
    inp = A.loss_inputs(64, 3, 2, 5, 9, 64)
    one = A.loss(inp)
    for gs in (0.5, 0.125):
        got = A.loss(inp, grad_scale=gs)
        assert got['rc'] == 0 and np.array_equal(got['loss'], one['loss'])
        for k in MAPS:
            assert np.array_equal(got['g_' + k], one['g_' + k] * np.float32(gs)), k
    assert all(np.abs(one['g_' + k]).max() > 0 for k in MAPS)


def test_loss_batch_strides():
    inp = A.loss_inputs(65, 3, 2, 9, 5, 9)
    dense = A.loss(inp)
    got = A.loss(inp, p_gap=7, t_planes=(1, 3), g_gap=13)
    check_loss(dense, ref_loss(inp))
    assert got['rc'] == 0 and np.array_equal(got['loss'], dense['loss']) and np.array_equal(got['stats'], dense['stats'])
    for k in MAPS:
        assert np.array_equal(got['g_' + k], dense['g_' + k]), k


def test_loss_without_gradients():
    inp = A.loss_inputs(66, 3, 2, 5, 9, 9)
    full = A.loss(inp)
    none = A.loss(inp, grads=False)                                   # the helper asserts that the gradient buffer stays 0xFF
    assert none['rc'] == 0 and np.array_equal(none['loss'], full['loss']) and none['g_heat'] is None


@pytest.mark.parametrize("kw", [
    dict(grads=(True, False, False, False, False, False)), dict(grads=(False, True, False, False, False, False)),
    dict(grads=(False, False, False, False, False, True)), dict(grads=(True, True, True, True, True, False)),
    dict(max_objs_arg=8193), dict(ws_short=1), dict(t_stride_arg=2 * 45 - 1), dict(p_stride_arg=3 * 45 - 1),
    dict(g_stride_arg=3 * 45 - 1), dict(null=('heat',)), dict(null=('reg',)),
    dict(null=('height',)), dict(null=('dim',)), dict(null=('rot',)), dict(null=('vel',))], ids=str)
def test_loss_rejections(kw):
    inp = A.loss_inputs(67, 3, 2, 5, 9, 8193 if 'max_objs_arg' in kw else 9)
    got = A.loss(inp, stats=(3.0, 4.0), **kw)
    assert got['rc'] != 0 and got['untouched']


def test_loss_stats_rejects_a_short_workspace_and_a_small_stride():
    inp = A.loss_inputs(68, 3, 2, 5, 9, 9)
    for kw in (dict(ws_short=1), dict(t_stride_arg=2 * 45 - 1)):
        got = A.loss(inp, **kw)
        assert got['stats_rc'] != 0 and got['rc'] != 0 and got['untouched'] and (got['stats'].view(np.uint32) == 0xFFFFFFFF).all()


def test_loss_is_deterministic():
    inp = A.shared_one_cell(64)
    a, b = A.loss(inp), A.loss(inp)
    assert np.array_equal(a['loss'], b['loss']) and all(np.array_equal(a['g_' + k], b['g_' + k]) for k in MAPS)
