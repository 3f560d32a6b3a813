"""CPU: the proposal-target contract and the rcnn losses against the reference head's ``assign_targets`` / ``get_loss``
(tests/golden/roi_targets_b2.npz, written by tests/golden/make_golden_roi_targets.py), the sampling rules on the golden's own
indices, the scenes of the GPU test against their margins, and the trainer's refusal.

Measured here against the fixture (the test prints the figures): with the sampling forced to the golden's ``roi_indices`` the numpy
statement gives every integer field, mask and copied row exactly; ``gt_iou_of_rois`` 0 (both round the same fp64 value once),
``rcnn_cls_labels`` 0, ``gt_of_rois`` 1.53e-5 (fp64 rotation rounded once against fp32 arithmetic: one fp32 ulp of the 148 m offset
between a far RoI and the GT row 0 it is assigned with overlap 0).  ``rcnn_losses`` against ``get_loss``: losses and both gradients 0 on this fixture.
A bound of 0 would pin one summation order and one vector width of exp / log / sigmoid / sqrt, so the bounds come from the number
format instead: 4 fp32 ulps of the total loss (2.4e-7 each at 2.44; the masked sums here run in another order than the reference's
gathered ones, and an earlier draw of the same scene differed by exactly one) and 4 fp32 ulps of the largest gradient entry, whose
entries are elementwise functions of the inputs divided by a count: another vector width of those functions may round an entry differently."""
import copy
import logging
import os

import numpy as np
import pytest
import torch

import roi_targets_reference as rt
from gdmae_hip import configs
from pcdet.models import build_network
from pcdet.models.roi_heads import proposal_targets as pt

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = {'gt_iou_of_rois': 0.0, 'rcnn_cls_labels': 0.0, 'gt_of_rois': 1.53e-5}
MEASURED_LOSS = 2.4e-7


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "roi_targets_b2.npz")))


@pytest.fixture(scope="module")
def detector():
    cfg, ds = configs.waymo_two_stage_cfg()
    return build_network(cfg, 3, ds, logging.getLogger("t")).eval()


def test_statement_reproduces_the_reference_targets(golden):
    z = golden
    P = rt.sampler_params(R=128)
    assert z["t_roi_indices"].shape == (2, 128) and z["rois_in"].shape == (2, 160, 7) and P['fg_per_image'] == 64
    out = rt.reference(z["rois_in"], z["roi_scores_in"], z["roi_labels_in"], z["gt_boxes"], None, None, P, forced_indices=z["t_roi_indices"])
    assert set(out) == {k[2:] for k in z if k.startswith("t_")} == set(pt.FIELDS)
    for k in ('roi_indices', 'roi_labels', 'reg_valid_mask'):
        assert np.array_equal(out[k], z["t_" + k]), k
    for k in ('rois', 'roi_scores', 'gt_of_rois_src'):
        assert out[k].tobytes() == z["t_" + k].astype(np.float32).tobytes(), k
    dev = {k: float(np.abs(out[k].astype(np.float64) - z["t_" + k]).max()) for k in MEASURED}
    print("deviation from the fixture:", dev)
    for k, m in MEASURED.items():
        assert dev[k] <= 4 * m, (k, dev[k])


def test_golden_indices_follow_the_sampling_rules(golden):
    """What the reference drew is one outcome of the contract's rules: the first f slots are distinct fg RoIs, the next h hard, the
    rest easy, with f and h as the rules give them."""
    z = golden
    P = rt.sampler_params(R=128)
    for b in range(2):
        best, _, _ = rt.match(z["rois_in"][b], z["roi_labels_in"][b], z["gt_boxes"][b], P['by_class'])
        iou = best.astype(np.float32)
        fg = iou >= np.float32(0.55)
        easy = iou < np.float32(0.1)
        hard = ~fg & ~easy
        n_fg, n_hard, n_easy = int(fg.sum()), int(hard.sum()), int(easy.sum())
        assert n_fg and n_hard and n_easy
        f = min(P['fg_per_image'], n_fg)
        h = min(int((128 - f) * 0.8), n_hard)
        assert h == min(P['hard_quota'][128 - f], n_hard)
        idx = z["t_roi_indices"][b]
        assert fg[idx[:f]].all() and len(set(idx[:f].tolist())) == f
        assert hard[idx[f:f + h]].all() and easy[idx[f + h:]].all()
        print("sample", b, "n_fg / n_hard / n_easy", n_fg, n_hard, n_easy, "f", f, "h", h)
    # the statement's own sampling obeys the same rules and is a function of (u_fg, u_bg) alone
    rng = np.random.RandomState(3)
    u_fg, u_bg = rng.random_sample((2, 160)).astype(np.float32), rng.random_sample((2, 128)).astype(np.float32)
    a = rt.reference(z["rois_in"], z["roi_scores_in"], z["roi_labels_in"], z["gt_boxes"], u_fg, u_bg, P)
    for b in range(2):
        best, _, _ = rt.match(z["rois_in"][b], z["roi_labels_in"][b], z["gt_boxes"][b], True)
        idx, c = pt.sample(best.astype(np.float32), u_fg[b], u_bg[b], P)
        assert np.array_equal(idx, a['roi_indices'][b])
        f, h = c['f'], c['h']
        fgl = np.nonzero(best.astype(np.float32) >= np.float32(0.55))[0]
        assert idx[:f].tolist() == sorted(fgl, key=lambda i: (u_fg[b, i], i))[:f]
        assert (best[idx[f:f + h]] < 0.55).all() and (best[idx[f:f + h]] >= 0.1).all() and (best[idx[f + h:]] < 0.1).all()


def test_package_clipping_agrees_with_the_oracle():
    rng = np.random.RandomState(5)
    worst = 0.0
    for _ in range(300):
        a = np.array([*rng.uniform(-2, 2, 2), 0, *rng.uniform(0.5, 5, 2), 1, rng.uniform(-4, 4)])
        b = np.array([*rng.uniform(-2, 2, 2), 0, *rng.uniform(0.5, 5, 2), 1, rng.uniform(-4, 4)])
        worst = max(worst, abs(pt.exact_bev_overlap(a, b) - rt.bev_overlap(a, b)))
    assert worst < 1e-12, worst


@pytest.mark.parametrize("name", sorted(rt.SCENES))
def test_scenes_meet_their_margins_and_cover_their_case(name):
    S, P, ref = rt.scene(name)                       # check_margins runs inside
    c = rt.counts(S, P)
    R = P['R']
    assert R == 16 and P['fg_per_image'] == 8 and all(v.shape[:2] == (S['rois'].shape[0], R) for v in ref.values())
    if name != 'strides':
        assert S['rois'].shape[1] <= 40 and S['gt_boxes'].shape[1] <= 12
    want = {'mixed': lambda: c[0]['n_fg'] > 8 > c[1]['n_fg'] > 0 and all(x['n_hard'] and x['n_easy'] for x in c) and (S['roi_labels'][1] == 0).any(),
            'no_boxes': lambda: not S['gt_boxes'][1].any() and c[1]['n_easy'] == S['rois'].shape[1],
            'all_fg': lambda: c[0]['n_hard'] + c[0]['n_easy'] == 0 and c[0]['f'] == 0,
            'one_bg_list': lambda: (c[0]['n_fg'] and c[0]['n_hard'] and not c[0]['n_easy'] and c[1]['n_fg'] and c[1]['n_easy'] and not c[1]['n_hard']
                                    and not c[2]['n_fg'] and not c[2]['n_easy']),
            'class_without_gt': lambda: c[0]['n_fg'] == 1 and (ref['roi_labels'] == 3).any() and (ref['gt_iou_of_rois'][ref['roi_labels'] == 3] == 0).all(),
            'duplicate_gt': lambda: c[0]['n_fg'] == 4,
            'equal_keys': lambda: c[0]['n_fg'] == 12 and ref['roi_indices'][0, :8].tolist() == sorted(ref['roi_indices'][0, :8].tolist()),
            'strides': lambda: S['rois'].shape[1] == 130 and S['gt_boxes'].shape[1] == 70 and c[0]['n_fg'] > 8,
            'any_class': lambda: c[0]['n_fg'] == 4 and not P['by_class'],
            'cls_labels': lambda: ref['rcnn_cls_labels'].dtype == np.int64 and set(np.unique(ref['rcnn_cls_labels'])) == {-1, 0, 1}}
    assert want[name](), c


def test_head_on_cpu_tensors_runs_the_statement(detector):
    S, P, _ = rt.scene('one_bg_list')
    head = copy.deepcopy(detector.roi_head)
    head.model_cfg.TARGET_CONFIG['ROI_PER_IMAGE'] = 16
    t = lambda a: torch.from_numpy(a.copy())      # noqa: E731
    bd = {'batch_size': 3, 'rois': t(S['rois']), 'roi_scores': t(S['roi_scores']), 'roi_labels': t(S['roi_labels']), 'gt_boxes': t(S['gt_boxes'])}
    td = head.proposal_targets(bd, t(S['u_fg']), t(S['u_bg']))
    own = pt.roi_targets_numpy(S['rois'], S['roi_scores'], S['roi_labels'], S['gt_boxes'], S['u_fg'], S['u_bg'], P)
    assert set(td) == set(pt.FIELDS)
    for k in pt.FIELDS:
        assert td[k].numpy().tobytes() == own[k].tobytes(), k
    for rows, name in ((1025, "RoIs"), (16, None)):
        if name:
            with pytest.raises(NotImplementedError, match=name):
                head.proposal_targets({**bd, 'rois': torch.zeros(3, rows, 7), 'roi_scores': torch.zeros(3, rows), 'roi_labels': torch.zeros(3, rows)},
                                      torch.zeros(3, rows), t(S['u_bg']))
    with pytest.raises(NotImplementedError, match="columns"):
        head.proposal_targets({**bd, 'rois': torch.zeros(3, 8, 9)}, t(S['u_fg']), t(S['u_bg']))


def test_rcnn_losses_match_the_reference(golden, detector):
    z = golden
    head = detector.roi_head
    ret = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("t_")}
    cls, reg = torch.from_numpy(z["rcnn_cls"]).requires_grad_(), torch.from_numpy(z["rcnn_reg"]).requires_grad_()
    loss, tb = head.rcnn_losses(dict(ret, rcnn_cls=cls, rcnn_reg=reg, batch_size=2))
    loss.backward()
    got = np.array([tb['rcnn_loss_cls'], tb['rcnn_loss_reg'], tb['rcnn_loss_corner'], tb['rcnn_loss']])
    d_loss = float(np.abs(got - z["losses"]).max())
    d_cls, d_reg = float(np.abs(cls.grad.numpy() - z["grad_cls"]).max()), float(np.abs(reg.grad.numpy() - z["grad_reg"]).max())
    print(f"losses {got.tolist()} deviation {d_loss:.3e}; gradients: cls {d_cls:.3e} reg {d_reg:.3e}")
    assert abs(float(loss.detach()) - tb['rcnn_loss']) < 1e-6 and all(isinstance(v, float) for v in tb.values())
    assert d_loss <= 4 * MEASURED_LOSS
    assert d_cls <= 4 * np.spacing(np.abs(z["grad_cls"]).max()) and d_reg <= 4 * np.spacing(np.abs(z["grad_reg"]).max())
    # without a fg row the regression and the corner loss are exactly 0 and carry no gradient
    ret0 = dict(ret, reg_valid_mask=torch.zeros_like(ret['reg_valid_mask']), rcnn_cls=cls.detach(), rcnn_reg=reg.detach().requires_grad_())
    _, tb0 = head.rcnn_losses(ret0)
    assert tb0['rcnn_loss_reg'] == 0.0 and tb0['rcnn_loss_corner'] == 0.0 and tb0['rcnn_loss'] == tb0['rcnn_loss_cls']
    # CrossEntropy on integer labels with ignored rows; other regression losses raise by name
    h2 = copy.deepcopy(head)
    h2.model_cfg.LOSS_CONFIG['CLS_LOSS'] = 'CrossEntropy'
    lab = torch.from_numpy(np.resize(np.array([1, 0, -1, 1]), 256))
    logits = torch.from_numpy(np.concatenate([z["rcnn_cls"], -z["rcnn_cls"]], axis=1))
    _, tbc = h2.rcnn_losses(dict(ret, rcnn_cls_labels=lab.view(2, 128), rcnn_cls=logits, rcnn_reg=reg.detach()))
    ok = lab >= 0
    want = float(torch.nn.functional.cross_entropy(logits[ok], lab[ok]))
    assert abs(tbc['rcnn_loss_cls'] - want) < 1e-6
    h2.model_cfg.LOSS_CONFIG['CLS_LOSS'] = 'BinaryCrossEntropy'
    h2.model_cfg.LOSS_CONFIG['REG_LOSS'] = 'WeightedL1Loss'
    with pytest.raises(NotImplementedError, match="WeightedL1Loss"):
        h2.rcnn_losses(dict(ret, rcnn_cls=cls.detach(), rcnn_reg=reg.detach()))


def test_trainer_refuses_joint_training_by_name(detector):
    from gdmae_hip.two_stage import SecondStageTrainer
    tr = SecondStageTrainer(copy.deepcopy(detector), rng=np.random.RandomState(0))
    assert tr.model.roi_head.training and not tr.model.dense_head.training and not tr.model.vfe.training
    assert all(not p.requires_grad for m in tr.model.module_list[:-1] for p in m.parameters())
    assert [id(p) for p in tr.trainable_parameters()] == [id(p) for p in tr.model.roi_head.parameters()]
    assert all(p.requires_grad for p in tr.trainable_parameters())
    tr.eval()
    tr.train()
    assert tr.model.roi_head.training and not tr.model.backbone_2d.training
    u_fg, u_bg = tr.draw(2, 5, 16, 'cpu')
    assert u_fg.shape == (2, 5) and u_bg.shape == (2, 16) and u_fg.dtype == torch.float32 and float(u_bg.max()) < 1
    want = np.random.RandomState(0)
    assert np.array_equal(u_fg.numpy(), want.random_sample((2, 5)).astype(np.float32)) and np.array_equal(u_bg.numpy(), want.random_sample((2, 16)).astype(np.float32))
    for layers in (None, ['DynVFE', 'SPTBackbone', 'SSTBEVBackbone']):
        d = copy.deepcopy(detector)
        d.model_cfg['FREEZE_LAYERS'] = layers
        with pytest.raises(NotImplementedError, match="joint training"):
            SecondStageTrainer(d)
    cfg, ds = configs.named_config("A")[:2]
    with pytest.raises(NotImplementedError, match="RoI head"):
        SecondStageTrainer(build_network(cfg, 3, ds, logging.getLogger("t")))
    # the detector's own training entry points keep refusing
    with pytest.raises(NotImplementedError, match="training"):
        tr.model({'batch_size': 1})
