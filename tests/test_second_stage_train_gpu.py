"""GPU: second-stage training of the shipped two-stage config through ``gdmae_hip.two_stage.SecondStageTrainer`` on a small synthetic
Waymo-range batch (B = 2, 16 beams) with hand-placed GT boxes: from given RoIs (GT boxes shifted into chosen IoU bands), against the
same head on the CPU, end to end through the frozen first stage, with an empty first stage, and two optimizer steps.

Measured on an MI355X (the test prints the figures): fp32 GPU-vs-CPU deviation of the training-mode head fed the device's sampled
targets and pooled features (256 RoIs, BatchNorm on batch statistics): 9.537e-6 on the losses (total 7.16), 4.156e-8 on the gradient
of the loss with respect to rcnn_cls (largest entry 3.8e-3) and 1.633e-5 with respect to rcnn_reg (largest entry 0.25); the test
asserts 4 x these, as tests/test_graph_rcnn_gpu.py does for the eval-mode head."""
import copy
import logging

import numpy as np
import pytest
import torch

import roi_targets_reference as rt
from gdmae_hip import configs, synth
from gdmae_hip.two_stage import SecondStageTrainer
from pcdet.models import build_network

pytestmark = pytest.mark.gpu

MEASURED_LOSS_DEV = 9.537e-6
MEASURED_GCLS_DEV = 4.156e-8
MEASURED_GREG_DEV = 1.633e-5

B = 2
GT_XY = [[(6.0, 5.0, 1), (-7.0, 8.0, 2), (12.0, -9.0, 3), (-13.0, -6.0, 1), (2.0, -14.0, 1)],
         [(-5.0, 6.0, 1), (9.0, 11.0, 3), (14.0, -4.0, 2), (-11.0, -12.0, 1)]]


def _model(seed=5):
    """The two-stage detector with seeded BatchNorm statistics everywhere and reg_layers weights large enough to move boxes."""
    cfg, ds = configs.waymo_two_stage_cfg()
    torch.manual_seed(seed)
    net = build_network(cfg, len(ds.class_names), ds, logging.getLogger("t"))
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(c, generator=g) * 1.0 + 0.5)
                m.weight.copy_(1.0 + 0.2 * torch.randn(c, generator=g))
                m.bias.copy_(0.2 * torch.randn(c, generator=g))
        net.roi_head.reg_layers.weight.copy_(torch.randn(net.roi_head.reg_layers.weight.shape, generator=g) * 0.05)
    return net.cuda().eval(), ds


@pytest.fixture(scope="module")
def setup():
    net, ds = _model()
    pts = synth.synth_batch(31, B, ds.point_cloud_range, beams=16, azimuths=1100, extra=3000, features=5)
    rng = np.random.RandomState(71)
    samples = []
    for b in range(B):
        gt = np.stack([rt.gt_box(rng, x, y, l) for x, y, l in GT_XY[b]])
        n = gt.shape[0]
        plan = [(k % n, rt.FG) for k in range(10)] + [(k % n, rt.HARD) for k in range(8)] + [(k % n, rt.EASY) for k in range(4)]
        rois, labels = rt.rois_for(rng, gt, plan, far=4)
        samples.append((gt, rois, labels))
    S = rt.assemble(rng, samples, G=6, M=28, R=128)
    P = rt.sampler_params(R=128)
    rt.check_margins(S, P)
    c = rt.counts(S, P)
    assert all(x['n_fg'] == 10 and x['n_hard'] == 8 and x['n_easy'] == 10 for x in c), c
    return net, ds, torch.from_numpy(pts).cuda(), {k: torch.from_numpy(v).cuda() for k, v in S.items()}


def _batch(points, S, with_rois=True):
    bd = {'points': points, 'batch_size': B, 'gt_boxes': S['gt_boxes'].clone()}
    if with_rois:
        bd.update(rois=S['rois'].clone(), roi_scores=S['roi_scores'].clone(), roi_labels=S['roi_labels'].clone())
    return bd


def _no_dropout(head):
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return head


def test_training_step_from_given_rois(setup):
    net, ds, points, S = setup
    tr = SecondStageTrainer(copy.deepcopy(net), rng=np.random.RandomState(3))
    head = tr.model.roi_head
    frozen = {k: v.clone() for k, v in tr.model.state_dict().items() if not k.startswith('roi_head.')}
    stats = {k: v.clone() for k, v in head.state_dict().items() if k.endswith('running_mean') or k.endswith('running_var')}
    assert len(frozen) > 50 and len(stats) >= 16
    torch.manual_seed(0)
    ret, tb, disp = tr(_batch(points, S))
    assert set(tb) == {'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss'} and disp == {}
    print("losses", tb)
    assert all(np.isfinite(v) and v > 0 for v in tb.values()) and abs(float(ret['loss'].detach()) - tb['rcnn_loss']) < 1e-5
    fr = head.forward_ret_dict
    assert fr['rois'].shape == (B, 128, 7) and fr['rcnn_cls'].shape == (B * 128, 1) and fr['rcnn_reg'].shape == (B * 128, 7)
    assert int(fr['reg_valid_mask'].sum()) >= 2 * 8 and int((fr['pooled_feats_local'].abs().sum(dim=(1, 2)) > 0).sum()) >= 100
    ret['loss'].backward()
    for n, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert float(head.reg_layers.weight.grad.abs().max()) > 0 and float(head.attn_gnn_layer.edge_layes[0][0].weight.grad.abs().max()) > 0
    for m in tr.model.module_list[:-1]:
        assert all(p.grad is None and not p.requires_grad for p in m.parameters())
    after = tr.model.state_dict()
    for k, v in frozen.items():
        assert torch.equal(after[k], v), k
    assert all(not torch.equal(after['roi_head.' + k], v) for k, v in stats.items())


def test_head_matches_the_cpu_on_the_same_targets(setup):
    net, ds, points, S = setup
    tr = SecondStageTrainer(copy.deepcopy(net))
    head = _no_dropout(tr.model.roi_head)
    head_cpu = copy.deepcopy(head).cpu().train()
    ret, tb, _ = tr(_batch(points, S), u_fg=S['u_fg'], u_bg=S['u_bg'])
    fr = head.forward_ret_dict
    fr['rcnn_cls'].retain_grad()
    fr['rcnn_reg'].retain_grad()
    ret['loss'].backward()
    # the device's targets are the contract's (the statement on the same inputs)
    z = {k: v.cpu().numpy() for k, v in S.items()}
    ref = rt.reference(z['rois'], z['roi_scores'], z['roi_labels'], z['gt_boxes'], z['u_fg'], z['u_bg'], rt.sampler_params(R=128))
    assert np.array_equal(fr['roi_indices'].cpu().numpy(), ref['roi_indices']) and np.array_equal(fr['reg_valid_mask'].cpu().numpy(), ref['reg_valid_mask'])
    feats = fr['pooled_feats_local'].cpu()
    cls, reg = head_cpu.heads(head_cpu.pooled_to_features(feats, B, 128), B, 128)
    cls.retain_grad()
    reg.retain_grad()
    cpu_ret = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in fr.items() if k not in ('rcnn_cls', 'rcnn_reg')}
    loss_cpu, tb_cpu = head_cpu.rcnn_losses(dict(cpu_ret, rcnn_cls=cls, rcnn_reg=reg))
    loss_cpu.backward()
    d_loss = max(abs(tb[k] - tb_cpu[k]) for k in tb)
    d_cls = float((fr['rcnn_cls'].grad.cpu() - cls.grad).abs().max())
    d_reg = float((fr['rcnn_reg'].grad.cpu() - reg.grad).abs().max())
    print(f"GPU-vs-CPU training head: losses {tb} / {tb_cpu}: {d_loss:.3e}; d loss / d rcnn_cls {d_cls:.3e} (largest {float(cls.grad.abs().max()):.3e}), "
          f"d loss / d rcnn_reg {d_reg:.3e} (largest {float(reg.grad.abs().max()):.3e})")
    assert d_loss <= 4 * MEASURED_LOSS_DEV and d_cls <= 4 * MEASURED_GCLS_DEV and d_reg <= 4 * MEASURED_GREG_DEV


def test_end_to_end_equals_the_first_stage_rois_fed_back(setup):
    net, ds, points, S = setup
    tr = SecondStageTrainer(copy.deepcopy(net), rng=np.random.RandomState(11))
    head = tr.model.roi_head
    seen = {}
    hook = tr.model.dense_head.register_forward_hook(
        lambda m, i, o: seen.update({k: o[k].clone() for k in ('rois', 'roi_scores', 'roi_labels')}))       # what the first stage proposed
    keep = lambda ret, tb: (ret['loss'].detach().clone(), tb, {k: v.detach().clone() for k, v in head.forward_ret_dict.items() if torch.is_tensor(v)})      # noqa: E731
    torch.manual_seed(4)                                                  # the dropout masks
    a = keep(*tr({'points': points, 'batch_size': B, 'gt_boxes': S['gt_boxes'].clone()})[:2])
    hook.remove()
    M = seen['rois'].shape[1]
    print("first stage proposes", (seen['roi_labels'] != 0).sum(dim=1).tolist(), "RoIs, padded to", M)
    assert 1 <= M <= 1024 and int((seen['roi_labels'] != 0).sum()) > 0 and seen['rois'].shape == (B, M, 7)
    # the trainer drew u_fg (B, M) first, then u_bg (B, 128); the same numbers and the same RoIs, given explicitly
    rng = np.random.RandomState(11)
    u_fg = torch.from_numpy(rng.random_sample((B, M)).astype(np.float32)).cuda()
    u_bg = torch.from_numpy(rng.random_sample((B, 128)).astype(np.float32)).cuda()
    calls = []
    hook = tr.model.dense_head.register_forward_hook(lambda m, i, o: calls.append(1))
    torch.manual_seed(4)
    b = keep(*tr({'points': points, 'batch_size': B, 'gt_boxes': S['gt_boxes'].clone(), **seen}, u_fg=u_fg, u_bg=u_bg)[:2])
    hook.remove()
    assert not calls                                                      # the first stage's head was skipped
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and set(a[2]) == set(b[2])
    for k, v in a[2].items():
        assert torch.equal(v, b[2][k]), k
    assert bool(torch.isfinite(a[0]))


def test_empty_first_stage_gives_easy_background_only(setup):
    net, ds, points, S = setup
    tr = SecondStageTrainer(copy.deepcopy(net), rng=np.random.RandomState(1))
    with torch.no_grad():
        for sep in tr.model.dense_head.heads_list:
            sep.hm[-1].weight.zero_()
            sep.hm[-1].bias.fill_(-20.0)
    bd = {'points': points, 'batch_size': B, 'gt_boxes': S['gt_boxes'].clone()}
    ret, tb, _ = tr(bd)
    fr = tr.model.roi_head.forward_ret_dict
    assert not bool(fr['roi_labels'].any()) and not bool(fr['rois'].any()) and not bool(fr['gt_iou_of_rois'].any())
    assert not bool(fr['reg_valid_mask'].any()) and not bool(fr['rcnn_cls_labels'].any()) and not bool(fr['roi_indices'].any())
    assert tb['rcnn_loss_reg'] == 0.0 and tb['rcnn_loss_corner'] == 0.0 and np.isfinite(tb['rcnn_loss_cls']) and tb['rcnn_loss_cls'] > 0
    ret['loss'].backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in tr.trainable_parameters() if p.grad is not None)


def test_two_optimizer_steps_lower_the_loss(setup):
    net, ds, points, S = setup
    tr = SecondStageTrainer(copy.deepcopy(net))
    opt = torch.optim.Adam(tr.trainable_parameters(), lr=1e-3)
    losses = []
    for step in range(3):
        torch.manual_seed(8)                                              # a fixed objective: the same dropout masks
        ret, tb, _ = tr(_batch(points, S), u_fg=S['u_fg'], u_bg=S['u_bg'])
        losses.append(tb['rcnn_loss'])
        if step < 2:
            opt.zero_grad()
            ret['loss'].backward()
            opt.step()
    print("loss over two Adam steps:", losses)
    assert losses[2] < losses[0] and np.isfinite(losses).all()
