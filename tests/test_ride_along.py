"""Launch-count switches of the encoder / conv-block backward and of the stage forward leave every bit where it was: the reductions that
ride along with the launch that follows them (GDMAE_LAYER_TAIL_RIDES, GDMAE_DW_REDUCE_RIDES: DESIGN section 9) are the same sums in the same
order as the launches of their own.  The switches are read once per process, so every setting is a subprocess that runs one bench-mode train
step (flat optimizer, bf16 autocast, fused layers) on a golden case's inputs and prints a digest of the loss and of the whole flat gradient."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEP = r'''
import hashlib, logging, os, sys
REPO = sys.argv[1]
sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), os.path.join(REPO, "tests")]
import numpy as np, torch
from helpers import load_case
from oracle import gdmae_oracle as orc          # test infrastructure: seeded parameters only
from gdmae_hip import configs, optim
from pcdet.models import build_network
dev = torch.device("cuda:0")
z, ds, cfg, shapes = load_case(sys.argv[2])
torch.manual_seed(0)
net = build_network(cfg, len(ds.class_names), ds, logging.getLogger("t")).to(dev)
net.load_state_dict(orc.seeded_state_dict(shapes, seed=int(z["seed"])), strict=False)
net.train()
opt = optim.FlatAdamOneCycle(net, configs.optimization_cfg(8), total_steps=10)
opt.zero_grad()
bd = {"points": torch.from_numpy(z["points"]).to(dev), "batch_size": int(z["batch_size"]), "mae_noise": torch.from_numpy(z["noise"]).to(dev)}
with torch.autocast("cuda", dtype=torch.bfloat16):
    ret, _, _ = net(bd)
ret["loss"].backward()
torch.cuda.synchronize()
g = opt.flat_grad.detach().cpu().numpy()
assert np.isfinite(g).all() and float(np.abs(g).sum()) > 0
print("DIGEST", float(ret["loss"]).hex(), hashlib.sha256(g.tobytes()).hexdigest())
'''


def _digest(case, env_extra):
    env = dict(os.environ)
    for k in ("GDMAE_LAYER_TAIL_RIDES", "GDMAE_DW_REDUCE_RIDES"):
        env.pop(k, None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", STEP, REPO, case], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("DIGEST")]
    assert len(lines) == 1, out.stdout[-2000:]
    return lines[0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["waymo_b1"])
def test_ride_along_switches_are_bit_identical(case):
    base = _digest(case, {})
    assert _digest(case, {}) == base, "the step itself is not bit-repeatable"
    for env in ({"GDMAE_LAYER_TAIL_RIDES": "0"}, {"GDMAE_DW_REDUCE_RIDES": "0"}, {"GDMAE_LAYER_TAIL_RIDES": "0", "GDMAE_DW_REDUCE_RIDES": "0"}):
        assert _digest(case, env) == base, env


@pytest.mark.gpu
def test_plan_issued_under_the_decoder_convolution():
    """SPTBackboneMAE.prefetch_plan_under_decoder: the next batch's plan is issued from inside the current forward (right before the tile
    convolution), finish() returns the plan prefetch_plan() builds, and a forward on it gives the loss of the inline plan, bit for bit."""
    import logging
    sys.path[:0] = [REPO, os.path.join(REPO, "gd-mae_amd"), os.path.join(REPO, "tests")]
    import torch
    from helpers import load_case
    from oracle import gdmae_oracle as orc
    from gdmae_hip import decoder as gdec
    from pcdet.models import build_network
    dev = torch.device("cuda:0")
    z, ds, cfg, shapes = load_case("waymo_b1")
    torch.manual_seed(0)
    net = build_network(cfg, len(ds.class_names), ds, logging.getLogger("t")).to(dev)
    net.load_state_dict(orc.seeded_state_dict(shapes, seed=int(z["seed"])), strict=False)
    net.train()
    pts, B = torch.from_numpy(z["points"]).to(dev), int(z["batch_size"])
    noise = torch.from_numpy(z["noise"]).to(dev)
    noise_cap = torch.cat([noise, torch.rand(pts.shape[0] - noise.numel(), device=dev)])
    bb = net.backbone_3d
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ref, _, _ = net({"points": pts, "batch_size": B, "mae_noise": noise})
        pf = bb.prefetch_plan_under_decoder(pts, B, noise=noise_cap)
        assert bb._pre_conv_hook is not None and not hasattr(gdec, "PRE_CONV_HOOK")      # on the module: no process-global hook
        issued = []
        real = bb.prefetch_plan
        bb.prefetch_plan = lambda *a, **k: (issued.append(1), real(*a, **k))[1]
        net({"points": pts, "batch_size": B, "mae_noise": noise})            # the forward that carries the issue
        assert bb._pre_conv_hook is None and issued == [1], "the forward did not issue the plan"
        bb.prefetch_plan = real
        vox, plan = pf.finish()
        out, _, _ = net({"points": pts, "batch_size": B, "_gdmae_vox": vox, "_gdmae_plan": plan})
    assert float(out["loss"]) == float(ref["loss"])
    # a forward that never reaches the tile convolution: finish() issues the plan itself
    pf2 = bb.prefetch_plan_under_decoder(pts, B, noise=noise_cap)
    vox2, plan2 = pf2.finish()
    assert bb._pre_conv_hook is None
    # a second model's forward does not fire this model's pending hook
    pf3 = bb.prefetch_plan_under_decoder(pts, B, noise=noise_cap)
    net2 = build_network(cfg, len(ds.class_names), ds, logging.getLogger("t")).to(dev).train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        net2({"points": pts, "batch_size": B, "mae_noise": noise})
    assert bb._pre_conv_hook is not None
    pf3.finish()
    assert bb._pre_conv_hook is None
    assert torch.equal(vox2.pillar_cell, vox.pillar_cell) and torch.equal(plan2.mask, plan.mask)
