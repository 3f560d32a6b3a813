"""Seeded parameters AND BatchNorm running statistics of the GraphRCNNHead parity fixture (no imports beyond torch: used by the
tests and by tests/golden/make_golden_roi_head.py on the reference module)."""
import torch

from head_seed import seeded_head_state


def seeded_roi_head_state(net, seed):
    """``seeded_head_state`` for the parameters; running means N(0, 0.1), running variances |N(0, 0.25)| + 0.5, in state_dict order."""
    sd = seeded_head_state(net, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    for k, v in net.state_dict().items():
        if k.endswith("running_mean"):
            sd[k] = torch.randn(tuple(v.shape), generator=g) * 0.1
        elif k.endswith("running_var"):
            sd[k] = (torch.randn(tuple(v.shape), generator=g) * 0.5).abs() + 0.5
    return sd
