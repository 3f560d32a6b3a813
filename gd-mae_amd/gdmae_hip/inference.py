"""Inference engine of the fine-tuned detectors: DynVFE -> SPTBackbone -> SSTBEVBackbone, then CenterHead (``CenterPoint``),
AnchorHeadSingle (``PointPillar``, the shipped KITTI fine-tune config) or CenterHead + GraphRCNNHead (``GraphRCNN``, the shipped
two-stage config).

    engine = compile_detector(model)           # model: CenterPoint / PointPillar / GraphRCNN from build_network, .eval(), on the GPU
    boxes, recall = engine(batch_dict)         # what model(batch_dict) returns in eval mode
    maps = engine.head_maps(batch_dict)        # per-head prediction maps (+ .spatial_features_2d, ...) of the first stage
    out = engine.refine(batch_dict)            # GraphRCNN only: the second stage on RoIs the caller supplies

The two-stage variant runs the first stage as the CenterPoint engine does, pools the RoIs' points with ``gdmae_roi_dfvs_pool`` and
runs the whole head behind the pooling - graph network, shared layer, heads, box decoding, score fusion - in the two launches of
``gdmae_roi_graph_forward`` (csrc/roi_graph.hip); ``post_processing`` takes its ``NMS: False`` branch.

The trunk (everything up to the channels-last bf16 BEV map) is shared; the head is a variant.  The anchor variant never writes the
dense per-anchor arrays: ``gdmae_anchor_head_infer`` goes from the BEV map to the anchors at or above SCORE_THRESH (score, label,
decoded box, in anchor order) in two launches, and the top-k / NMS tail of ``post_processing`` runs on those survivors only.
``engine.detect(batch_dict)`` (all three engines) runs that tail for the whole batch on the device and returns padded tensors;
``engine.detect(batch_dict, recall=record)`` also adds the batch's recall figures to a ``gdmae_hip.evaluation.RecallRecord``.

In evaluation mode every BatchNorm is a constant per-channel affine: a = gamma / sqrt(running_var + eps), b = beta - a running_mean.
``compile_detector`` folds it into the weights of the product in front of it (W' = a W per output channel, computed in fp64 and
rounded once to the operand type when the image is packed) and keeps b in fp32 for the product's epilogue, so that every
product -> BatchNorm -> ReLU (-> + shortcut) block is ONE launch of libgdmae_hip.so and no framework convolution, BatchNorm, ReLU or
GEMM kernel runs.  ``model.eval(); model(batch_dict)`` is not changed by any of this: it stays the exact (fp32) mode.

The engine holds its own folded / packed copies.  It never writes to the model, runs under ``torch.no_grad()`` whatever the caller's
grad mode, and refuses to run on stale images: the ``_version`` counters of every parameter and buffer are recorded at compile /
``refresh()`` and compared at every call (optimizer steps of ``gdmae_hip.optim.FlatAdamOneCycle``, which updates its flat buffer
without touching the counters, are seen through ``optim.GENERATION``).  Anything the kernels do not cover raises NotImplementedError.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import decoder as gdec
from . import encoder as genc
from . import lib as L
from . import optim as goptim
from . import packing
from . import plan as gplan

BF16 = torch.bfloat16


def _pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def _no(msg: str):
    raise NotImplementedError("gdmae_hip.inference: " + msg)


def fold_bn(bn, n_out: int, dev):
    """(a, b) in fp64 of a BatchNorm in evaluation mode; bn = None: the identity."""
    if bn is None:
        return torch.ones(n_out, dtype=torch.float64, device=dev), torch.zeros(n_out, dtype=torch.float64, device=dev)
    if isinstance(bn, nn.SyncBatchNorm):
        _no("SyncBatchNorm (convert the model back with the statistics it holds)")
    if not isinstance(bn, (nn.BatchNorm1d, nn.BatchNorm2d)):
        _no(f"{type(bn).__name__} where a BatchNorm is expected")
    if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
        _no("a BatchNorm without running statistics has no constant affine in evaluation mode")
    if bn.num_features != n_out:
        _no("BatchNorm width does not match the product in front of it")
    var, mean = bn.running_var.detach().double(), bn.running_mean.detach().double()
    gamma = bn.weight.detach().double() if bn.affine else torch.ones_like(var)
    beta = bn.bias.detach().double() if bn.affine else torch.zeros_like(var)
    a = gamma / torch.sqrt(var + float(bn.eps))
    return a, beta - a * mean


def _block(seq, kind):
    """(product, BatchNorm) of a Sequential(product, BatchNorm, ReLU)."""
    mods = list(seq.children())
    if len(mods) != 3 or not isinstance(mods[0], kind) or not isinstance(mods[2], nn.ReLU):
        _no(f"expected Sequential({kind.__name__}, BatchNorm, ReLU), got {[type(m).__name__ for m in mods]}")
    return mods[0], mods[1]


def _record(model, recall, batch_dict):
    """The ``RecallRecord`` a ``detect`` call updates, or None (``evaluation.post_cfg_record``: thresholds checked before anything runs)."""
    if recall is None:
        return None
    from . import evaluation
    return evaluation.post_cfg_record(model.model_cfg.POST_PROCESSING, recall, batch_dict)


class _Dense:
    """One Conv2d(3 x 3, stride 1, padding = dilation) launch: packed image of W' and the padded fp32 bias."""

    def __init__(self, conv: nn.Conv2d, bn, relu: bool):
        if not isinstance(conv, nn.Conv2d):
            _no(f"{type(conv).__name__} where a Conv2d is expected")
        d = int(conv.dilation[0])
        cin, cout = conv.in_channels, conv.out_channels
        if relu and cout % 32 != 0:
            _no(f"dense block with {cout} output channels (the next convolution reads channels in multiples of 32)")
        ok = (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.dilation == (d, d) and
              conv.padding == (d, d) and d in (1, 2) and conv.groups == 1 and conv.padding_mode == 'zeros' and cin % 32 == 0 and
              cin <= 1024 and cout <= 1024 and (d == 1 or (cin % 64 == 0 and cout % 64 == 0)))
        if not ok:
            _no(f"dense convolution {conv} (3 x 3, stride 1, padding = dilation in (1, 2), input channels in multiples of 32)")
        dev = conv.weight.device
        a, b = fold_bn(bn, cout, dev)
        w = (conv.weight.detach().double() * a.view(-1, 1, 1, 1)).float().contiguous()
        if conv.bias is not None:
            b = b + a * conv.bias.detach().double()
        self.cin, self.cout, self.cl, self.dil, self.relu = cin, cout, _pad32(cout), d, relu
        self.packed = torch.empty(L.load().gdmae_conv3x3_dense_packed_bytes(cin, cout), dtype=torch.uint8, device=dev)
        L.call("gdmae_conv3x3_dense_pack", L.ptr(w), cin, cout, d, 0, L.ptr(self.packed), L.stream())
        self.bias = torch.zeros(self.cl, dtype=torch.float32, device=dev)
        self.bias[:cout] = b.float()

    def __call__(self, x, shortcut=None):
        """x (B, H, W, cin) bf16 contiguous -> (B, H, W, pad32(cout)) bf16"""
        B, H, W, c = x.shape
        assert c == self.cin and x.dtype == BF16 and x.is_contiguous()
        y = torch.empty(B, H, W, self.cl, dtype=BF16, device=x.device)
        if self.relu:
            L.call("gdmae_conv3x3_dense_relu", L.ptr(x), B, H, W, self.cin, self.cl, self.dil, L.ptr(self.packed), L.ptr(self.bias),
                   None if shortcut is None else L.ptr(shortcut), L.ptr(y), L.stream())
        else:
            assert shortcut is None
            L.call("gdmae_conv3x3_dense", L.ptr(x), B, H, W, self.cin, self.cl, self.dil, L.ptr(self.packed), L.ptr(self.bias), L.ptr(y),
                   L.stream())
        return y


class _Sparse:
    """One sparse convolution + folded BatchNorm + ReLU launch."""

    def __init__(self, seq):
        from pcdet.utils.spconv_utils import SparseConvolution
        conv, bn = _block(seq, SparseConvolution)
        cout, cin = conv.out_channels, conv.in_channels
        if cin not in (128, 256) or cout not in (128, 256):
            _no(f"sparse convolution {cin} -> {cout} (channels must be 128 or 256)")
        a, b = fold_bn(bn, cout, conv.weight.device)
        w = (conv.weight.detach().double() * a.view(-1, 1, 1, 1)).float().contiguous()       # (cout, 3, 3, cin)
        self.packed, _ = packing.conv_pack_now(w)
        self.bias = b.float().contiguous()
        self.cin, self.cout, self.subm = cin, cout, conv.subm

    def __call__(self, x, nbr):
        n = nbr.shape[0]
        y = torch.empty(n, self.cout, dtype=BF16, device=x.device)
        if n:
            L.call("gdmae_spconv_bias_relu", L.ptr(x), int(x.dtype == torch.float32), L.ptr(nbr), L.ptr(self.packed), L.ptr(self.bias), n,
                   self.cin, self.cout, L.ptr(y), L.stream())
        return y


class _Stage:
    """The encoder layers of one SSTBlockV1 through gdmae_encoder_stage_fwd (no autograd node): x -> x + layers(x) in bf16."""

    def __init__(self, blk):
        self.layers = [(layer, k) for block in blk.encoder_blocks for k, layer in enumerate(block.encoder_list)]
        if not self.layers:
            _no("an SST block without encoder layers")
        self.bases, self.keep = [], []
        for layer, _ in self.layers:
            if layer.activation_name != "gelu":
                _no("encoder activation other than gelu")
            Win, bin_, tau, Wo, bo, W1, b1, W2, b2, g1, be1, g2, be2 = genc._plist(layer)
            c16 = lambda t: t.detach().to(BF16).contiguous()                       # noqa: E731
            f32 = lambda t: t.detach().float().clone().contiguous()                # noqa: E731
            ts = {"Win": c16(Win), "bin": c16(bin_), "Wo": c16(Wo), "bo": c16(bo), "W1": c16(W1), "b1": c16(b1), "W2": c16(W2), "b2": c16(b2),
                  "g1": f32(g1), "be1": f32(be1), "g2": f32(g2), "be2": f32(be2), "tau": f32(tau.reshape(1))}
            packed = packing.pack_now(f32(Win), f32(Wo), f32(W1), f32(W2))
            if packed is None:
                _no("encoder weights must be fp32 device tensors")
            ts["packed"] = packed
            a = L.LayerArgs()
            for k, t in ts.items():
                setattr(a, k, L.ptr(t))
            self.bases.append(a)
            self.keep.append(ts)
        l0 = self.layers[0][0]
        sa = l0.win_attn.self_attn
        self.nhead, self.tau_min, self.eps, self.ff = sa.num_heads, sa.tau_min, l0.norm1.eps, l0.linear1.weight.shape[0]
        self.input_layer = blk.sst_input_layer

    def __call__(self, x, wplans):
        n, d = x.shape
        dev = x.device
        if n == 0:
            return x.to(BF16)
        nl = len(self.layers)
        table = self.input_layer.pos_table(d, dev)
        sb, fb, _ = genc._layer_bytes(n, d, self.ff, self.nhead, 1)
        arr = (L.LayerArgs * nl)()
        for i, (_, k) in enumerate(self.layers):
            arr[i] = genc._call_args(self.bases[i], x, wplans[k % len(wplans)], table, self.nhead, self.tau_min, self.eps, BF16, self.ff)
        # the forward entry also writes what only a backward reads (log-sum-exp rows, LayerNorm statistics, pre-GELU rows): `saved`
        saved = torch.empty(nl, sb, dtype=torch.uint8, device=dev)
        scratch = torch.empty(fb, dtype=torch.uint8, device=dev)
        for i in range(nl):
            arr[i].saved, arr[i].scratch = saved[i].data_ptr(), scratch.data_ptr()
        fused = bool(L.load().gdmae_encoder_stage_fused(arr, nl))
        folded = fused and x.dtype == BF16
        res = torch.empty(n, d, dtype=BF16, device=dev)
        if fused:
            xin = x.contiguous() if folded else x.float().contiguous()
            out = res if folded else torch.empty(n, d, dtype=torch.float32, device=dev)
            for i in range(nl):
                arr[i].path = 1
                arr[i].x = xin.data_ptr() if i == 0 else None
            if folded:
                arr[0].x_bf16 = 1
                arr[nl - 1].res_out = res.data_ptr()
            else:
                arr[nl - 1].y = out.data_ptr()
        else:
            xin = x.float().contiguous()
            ys = torch.empty(nl, n, d, dtype=torch.float32, device=dev)
            for i in range(nl):
                arr[i].x = (xin if i == 0 else ys[i - 1]).data_ptr()
                arr[i].y = ys[i].data_ptr()
            out = ys[nl - 1]
        L.call("gdmae_encoder_stage_fwd", arr, nl, L.stream())
        if not folded:
            L.call("gdmae_add3_to", L.ptr(out), L.ptr(xin), 0, None, 0, out.numel(), L.ptr(res), 1, L.stream())
        return res


class HeadMaps(list):
    """The per-head prediction dicts (what ``CenterHead.generate_predicted_boxes`` takes; for the anchor head one dict with the
    ``cls_preds`` / ``box_preds`` / ``dir_cls_preds`` of its ``forward_ret_dict``) plus the maps in front of them."""
    spatial_features_2d = None
    spatial_features = None
    pillar_features = None
    voxel_coords = None


class DetectorEngine:
    """The shared trunk; ``CenterPointEngine`` / ``AnchorEngine`` add the head."""

    @staticmethod
    def HEAD():
        """the dense head class of the variant"""
        raise NotImplementedError

    def _refresh_head(self, dev):
        raise NotImplementedError

    def _check_stages(self, model):
        if getattr(model, "roi_head", None) is not None or getattr(model, "point_head", None) is not None:
            _no("two-stage heads")

    def __init__(self, model):
        from pcdet.models.backbones_3d.vfe.dyn_vfe import DynVFE
        from pcdet.models.backbones_3d.spt_backbone import SPTBackbone
        from pcdet.models.backbones_2d.sst_bev_backbone import SSTBEVBackbone
        if not next(model.parameters()).is_cuda:       # what is not covered first (NotImplementedError), then how it is called
            _no("the model must be on the GPU (the CenterPoint / PointPillar / GraphRCNN engines run on the library's kernels only)")
        if model.training:
            raise ValueError("gdmae_hip.inference: compile_detector needs the model in evaluation mode (call model.eval() first)")
        for name, kind in (("vfe", DynVFE), ("backbone_3d", SPTBackbone), ("backbone_2d", SSTBEVBackbone), ("dense_head", self.HEAD())):
            if not isinstance(getattr(model, name, None), kind):
                _no(f"model.{name} must be a {kind.__name__}")
        self._check_stages(model)
        self.model = model
        self.refresh()

    # ---- freshness -------------------------------------------------------------------------------------------------
    def _stamp(self):
        """What a call compares with compile / refresh() time: identity, version counter and storage address of every parameter and
        buffer the model holds NOW (a tensor replaced by assignment, an in-place update, a .to() / load that moved storage), and the
        count of FlatAdamOneCycle steps in this process.  Known gaps: a write through ``.data`` of the same storage bumps no counter
        and is not seen; the step count is process-wide, so a flat-optimizer step on ANY model makes every engine stale (it errs on
        the side of a refresh)."""
        ts = list(self.model.parameters()) + list(self.model.buffers())
        return (tuple((id(t), t._version, t.data_ptr()) for t in ts), goptim.GENERATION)

    def _check_fresh(self):
        if self.model.training:
            raise RuntimeError("gdmae_hip.inference: the model is in training mode; the engine serves model.eval()")
        if self._stamp() != self._stamped:
            raise RuntimeError("gdmae_hip.inference: the model's parameters or buffers changed since compile_detector / refresh(); "
                               "call engine.refresh() to rebuild the folded weight images")

    @torch.no_grad()
    def refresh(self):
        """(Re)build every folded, packed weight image from the model's current parameters and BatchNorm buffers."""
        m = self.model
        stamp = self._stamp()
        dev = next(m.parameters()).device
        # DynVFE: Linear (no bias) -> BatchNorm1d -> ReLU, twice
        mlp = m.vfe.dvfe_mlps[0]
        if len(mlp) != 6 or not isinstance(mlp[0], nn.Linear) or not isinstance(mlp[3], nn.Linear):
            _no("DynVFE with other than two Linear-BatchNorm-ReLU layers")
        l1, bn1, l2, bn2 = mlp[0], mlp[1], mlp[3], mlp[4]
        if l1.out_features != 64 or l2.in_features != 64 or l2.out_features != 128:
            _no(f"DynVFE layers {l1.out_features}, {l2.out_features} (the kernel takes 64 and 128)")
        vw = []
        for lin, bn in ((l1, bn1), (l2, bn2)):
            a, b = fold_bn(bn, lin.out_features, dev)
            w = (lin.weight.detach().double() * a.view(-1, 1)).float().contiguous()
            if lin.bias is not None:
                b = b + a * lin.bias.detach().double()
            vw += [w, b.float().contiguous()]
        self.vfe_w = vw
        # encoder stages + the five sparse convolutions
        bb = m.backbone_3d
        self.stages = []
        for blk in bb.sst_blocks:
            self.stages.append((None if blk.conv_down is None else _Sparse(blk.conv_down), _Stage(blk), _Sparse(blk.conv_out)))
        # decoder: ConvTranspose2d(k = s) rows per source stage, one constant background row, conv_out
        self.deblocks = []
        bg = []
        for blk in bb.deblocks:
            dc, bn = _block(blk, nn.ConvTranspose2d)
            s = int(dc.stride[0])
            cin, cout = dc.in_channels, dc.out_channels
            if not (dc.kernel_size == (s, s) and dc.stride == (s, s) and dc.bias is None and dc.padding == (0, 0) and dc.output_padding == (0, 0)
                    and cin in (128, 256) and cout == 128 and s in (1, 2, 4) and dc.groups == 1):
                _no(f"decoder deblock {dc}")
            a, b = fold_bn(bn, cout, dev)
            w = (dc.weight.detach().double() * a.view(1, -1, 1, 1)).float().contiguous()
            nb = L.load().gdmae_deconv_rows_packed_bytes(cin, cout, s)
            pf = torch.empty(nb, dtype=torch.uint8, device=dev)
            pb = torch.empty(nb, dtype=torch.uint8, device=dev)
            L.call("gdmae_deconv_rows_pack", L.ptr(w), cin, cout, s, L.ptr(pf), L.ptr(pb), L.stream())
            self.deblocks.append((pf, b.float().contiguous(), cin, cout, s))
            bg.append(torch.clamp_min(b, 0.0))
        self.dec_bg = torch.cat(bg).float().to(BF16).contiguous()           # an empty site of branch i holds relu(b_i), not zero
        self.dec_ones = torch.ones(128, dtype=torch.float32, device=dev)
        self.dec_sources = [int(src[-1]) - 1 for src in bb.model_cfg.FEATURES_SOURCE]
        conv, bn = _block(bb.conv_out, nn.Conv2d)
        self.dec_out = _Dense(conv, bn, True)
        if self.dec_out.cin != self.dec_bg.numel():
            _no("decoder conv_out width")
        # BEV backbone
        self.bev = []
        c = self.dec_out.cout
        for i, blk in enumerate(m.backbone_2d.conv_layer):
            conv, bn = _block(blk, nn.Conv2d)
            if conv.in_channels != c:
                _no("BEV block input width does not follow the block before it")
            self.bev.append((_Dense(conv, bn, True), conv.out_channels == c and i in m.backbone_2d.conv_shortcut))
            c = conv.out_channels
        self.bev_out = c
        self._refresh_head(dev)
        self._stamped = stamp
        return self

    # ---- one forward -----------------------------------------------------------------------------------------------
    def _trunk(self, batch_dict):
        """-> (B, x2 (B, H, W, c) channels-last bf16 BEV map, sf: the decoder's map, pillar features, the voxelisation).  Called under
        no_grad and with autocast disabled."""
        from pcdet.models.backbones_3d.spt_backbone import stage_plan_args
        m = self.model
        vfe, bb = m.vfe, m.backbone_3d
        B = int(batch_dict['batch_size'])
        vox = batch_dict.get('_gdmae_vox', None)
        if vox is None:
            vox = gplan.voxelize(batch_dict['points'], vfe.point_cloud_range, vfe.voxel_size, vfe.grid_size, B)
        if not 3 <= vox.n_cols - 1 <= 5 or vox.points_pm is None:
            _no("points with 3 to 5 features in pillar-major order")
        dev = vox.voxel_coords.device
        pf = torch.empty(vox.M, 128, dtype=torch.float32, device=dev)
        w1, b1, w2, b2 = self.vfe_w
        L.call("gdmae_vfe_infer", L.ptr(vox.points_pm), L.ptr(vox.voxel_coords), L.ptr(vox.row_pillar), L.ptr(vox.pillar_mean), int(vox.N),
               int(vox.M), vox.n_cols, L.host_f32(vox.lo), L.host_f32(vox.vs), L.ptr(w1), L.ptr(b1), 64, L.ptr(w2), L.ptr(b2), 128, L.ptr(pf),
               L.stream())
        ep = gplan.encoder_plan(vox, *stage_plan_args(bb.model_cfg.SST_BLOCK_LIST), keep_frac=None)
        x, si, hidden = pf, 0, []
        for down, stage, conv_out in self.stages:
            if down is not None:
                si += 1
                x = down(x, ep.stages[si].nbr_down)
            sp = ep.stages[si]
            x = conv_out(stage(x, sp.windows), sp.nbr_subm)
            hidden.append((x, sp))
        # decoder: the concatenated map = the constant row everywhere + relu(P' + b_i) at the sites the tokens cover
        srcs = [hidden[i] for i in self.dec_sources]
        s0 = self.deblocks[0][4]
        Y, X = srcs[0][1].Y * s0, srcs[0][1].X * s0
        ctot = self.dec_bg.numel()
        Z = torch.empty(B * Y * X, ctot, dtype=BF16, device=dev)
        L.call("gdmae_fill_rows", L.ptr(self.dec_bg), B * Y * X, ctot, 2, L.ptr(Z), L.stream())
        col0 = 0
        for (pf_img, b, cin, cout, s), (h, sp) in zip(self.deblocks, srcs):
            if sp.Y * s != Y or sp.X * s != X or sp.B != B:
                _no("decoder sources of different full-resolution sizes")
            n = h.shape[0]
            if n:
                P = torch.empty(n * s * s, cout, dtype=BF16, device=dev)
                L.call("gdmae_deconv_rows_fwd", L.ptr(h), n, cin, cout, s, L.ptr(pf_img), L.ptr(P), L.stream())
                sites = gdec.upsampled_sites(sp, s, Y, X).contiguous()
                L.call("gdmae_rows_affine_relu_scatter", L.ptr(P), 1, L.ptr(sites), n * s * s, cout, L.ptr(self.dec_ones), L.ptr(b), L.ptr(Z), 1,
                       ctot, col0, L.stream())
            col0 += cout
        sf = self.dec_out(Z.view(B, Y, X, ctot))
        x2 = sf
        for conv, shortcut in self.bev:
            x2 = conv(x2, x2 if shortcut else None)
        return B, x2, sf, pf, vox

    @staticmethod
    def _with_maps(out: HeadMaps, x2, sf, pf, vox) -> HeadMaps:
        out.spatial_features_2d = x2.permute(0, 3, 1, 2)
        out.spatial_features = sf.permute(0, 3, 1, 2)
        out.pillar_features = pf
        out.voxel_coords = vox.voxel_coords
        return out


class CenterPointEngine(DetectorEngine):
    @staticmethod
    def HEAD():
        from pcdet.models.dense_heads.center_head import CenterHead
        return CenterHead

    def _refresh_head(self, dev):
        m, c = self.model, self.bev_out
        hd = m.dense_head
        conv, bn = _block(hd.shared_conv, nn.Conv2d)
        self.shared = _Dense(conv, bn, True)
        if self.shared.cin != c:
            _no("shared_conv input width does not follow the BEV backbone")
        self.heads = []
        for head in hd.heads_list:
            branches = []
            for name in head.sep_head_dict:
                seq = list(getattr(head, name).children())
                ops, w = [], self.shared.cout
                for layer in seq[:-1]:
                    conv, bn = _block(layer, nn.Conv2d)
                    ops.append(_Dense(conv, bn, True))
                    if ops[-1].cin != w:
                        _no(f"head branch {name}: channel widths do not chain")
                    w = ops[-1].cout
                if not isinstance(seq[-1], nn.Conv2d):
                    _no("head branch must end in a Conv2d")
                ops.append(_Dense(seq[-1], None, False))
                if ops[-1].cin != w:
                    _no(f"head branch {name}: channel widths do not chain")
                branches.append((name, ops))
            self.heads.append(branches)

    @torch.no_grad()
    def head_maps(self, batch_dict) -> HeadMaps:
        self._check_fresh()
        with torch.autocast("cuda", enabled=False):
            B, x2, sf, pf, vox = self._trunk(batch_dict)
            xs = self.shared(x2)
            out = HeadMaps()
            for branches in self.heads:
                pd = {}
                for name, ops in branches:
                    y = xs
                    for op in ops:
                        y = op(y)
                    pd[name] = y[..., :ops[-1].cout].permute(0, 3, 1, 2)
                out.append(pd)
        return self._with_maps(out, x2, sf, pf, vox)

    @torch.no_grad()
    def __call__(self, batch_dict):
        maps = self.head_maps(batch_dict)
        B = int(batch_dict['batch_size'])
        m = self.model
        with torch.autocast("cuda", enabled=False):
            boxes = m.dense_head.generate_predicted_boxes(B, maps)
            bd = {'final_box_dicts': boxes, 'batch_size': B}
            if 'gt_boxes' in batch_dict:
                bd['gt_boxes'] = batch_dict['gt_boxes']
            return m.post_processing(bd)

    @torch.no_grad()
    def detect(self, batch_dict, recall=None):
        """``head_maps``, then the batched tail (``CenterHead.generate_predicted_boxes_batched``: three launches for all samples and
        classes): pred_boxes (B, n, 7 | 9), pred_scores (B, n), pred_labels (B, n) int64, num (B) int32 on the device, rows at or beyond
        num[b] zero; n depends on the config only.  Nothing is read on the host after the trunk;
        ``CenterHead.padded_to_pred_dicts`` gives the per-sample list of ``engine(batch_dict)``.  ``recall``: a
        ``gdmae_hip.evaluation.RecallRecord`` that receives the batch's recall figures (two more launches, still no host read) when
        ``batch_dict`` has ``gt_boxes``; without either, no recall record is computed."""
        rec = _record(self.model, recall, batch_dict)
        maps = self.head_maps(batch_dict)
        with torch.autocast("cuda", enabled=False):
            out = self.model.dense_head.generate_predicted_boxes_batched(int(batch_dict['batch_size']), maps)
            if rec is not None:
                rec.update(out['pred_boxes'], out['num'], batch_dict['gt_boxes'])
            return out


ROI_GRAPH_CONFIG = {'IN_DIM': 11, 'MLPS': [32, 32, 64], 'CALIB_DIM': 64, 'EXP_MLPS': [512], 'OUT_DIM': 256, 'K': 8, 'USE_FEATS_DIS': False,
                    'USE_REDUCTION': True, 'USE_SHORT_CUT': True}


def fold_roi_head(head):
    """The ``folded`` fp32 buffer of ``gdmae_roi_graph_pack`` (include/gdmae_hip.h) from a ``GraphRCNNHead`` in eval mode: every
    BatchNorm folded in fp64 into the product in front of it, an edge layer split into P = a W_nbr and Q = a (W_ctr - W_nbr).
    Anything the kernels are not specialised to is refused by name."""
    from pcdet.models.roi_heads.graphrcnn_head import GraphRCNNHead
    if not isinstance(head, GraphRCNNHead):
        _no(f"model.roi_head must be a GraphRCNNHead, not {type(head).__name__}")
    gnn_cfg, gnn = head.model_cfg.ATTN_GNN_CONFIG, head.attn_gnn_layer
    for key, want in ROI_GRAPH_CONFIG.items():
        got = gnn_cfg.get(key, None)
        got = list(got) if isinstance(got, (list, tuple)) else got
        if got != want:
            _no(f"ROI_HEAD.ATTN_GNN_CONFIG.{key}: {got} (the second-stage kernels are specialised to {want})")
    if gnn.reduction is None or gnn.shortcut is None:
        _no("ROI_HEAD.ATTN_GNN_CONFIG.USE_REDUCTION / USE_SHORT_CUT: False (the second-stage kernels include both blocks)")
    pool = head.roilocal_dfvs_pool3d_layer
    if int(pool.num_fps_points) != 256 or int(head.model_cfg.DFVS_CONFIG.NUM_FPS_POINTS) != 256:
        _no(f"ROI_HEAD.DFVS_CONFIG.NUM_FPS_POINTS: {pool.num_fps_points} (the second-stage kernels take 256 points per RoI)")
    if head.num_class != 1:
        _no(f"a RoI head with num_class = {head.num_class} (the second-stage kernels are class-agnostic: CLASS_AGNOSTIC True)")
    if head.box_coder.code_size != 7:
        _no("a RoI head box coder with other than 7 codes")
    dev = head.cls_layers.weight.device

    def conv(c, cout, cin, bias):
        kind = nn.Conv2d if c.weight.dim() == 4 else nn.Conv1d
        if not isinstance(c, kind) or tuple(c.weight.shape[:2]) != (cout, cin) or c.weight[0, 0].numel() != 1 or (c.bias is not None) != bias:
            _no(f"second-stage layer {c} where a 1 x 1 convolution {cin} -> {cout} ({'with' if bias else 'no'} bias) is expected")
        return c.weight.detach().double().reshape(cout, cin), (c.bias.detach().double() if bias else None)

    out = []
    if gnn.k != 8 or len(gnn.edge_layes) != 3:
        _no("ROI_HEAD.ATTN_GNN_CONFIG: K / MLPS of the built graph network differ from the config")
    cin = 11
    for seq, c in zip(gnn.edge_layes, (32, 32, 64)):
        cv, bn = _block(seq, nn.Conv2d)
        w, _ = conv(cv, c, 2 * cin, False)
        a, b = fold_bn(bn, c, dev)
        out += [a[:, None] * w[:, :cin], a[:, None] * (w[:, cin:] - w[:, :cin]), b]
        cin = c
    cal = list(gnn.calib.children())
    if len(cal) != 4 or not isinstance(cal[2], nn.ReLU):
        _no("calib block other than Conv1d, BatchNorm1d, ReLU, Conv1d")
    w, _ = conv(cal[0], 64, 128, False)
    a, b = fold_bn(cal[1], 64, dev)
    out += [a[:, None] * w, b, *conv(cal[3], 128, 64, True)]
    for seq, co, ci in ((gnn.expansion, 512, 128), (gnn.reduction, 256, 512)):
        cv, bn = _block(seq, nn.Conv1d)
        w, _ = conv(cv, co, ci, False)
        a, b = fold_bn(bn, co, dev)
        out += [a[:, None] * w, b]
    sc = gnn.shortcut
    a, b = fold_bn(sc.norm1, 256, dev)
    out += [2.0 * a, b, *conv(sc.conv1, 256, 256, True), *conv(sc.conv2, 256, 256, True), *fold_bn(sc.norm2, 256, dev)]      # x + dropout1(x) = 2 x
    cv, bn = _block(head.shared_fc_layer, nn.Conv1d)
    w, _ = conv(cv, 256, 256, False)
    a, b = fold_bn(bn, 256, dev)
    wc, bc = conv(head.cls_layers, 1, 256, True)
    wr, br = conv(head.reg_layers, 7, 256, True)
    out += [a[:, None] * w, b, torch.cat([wc, wr]), torch.cat([bc, br])]
    flat = torch.cat([t.reshape(-1) for t in out]).float().contiguous()
    if flat.numel() != L.load().gdmae_roi_graph_folded_floats():
        _no("second-stage weights do not fill the kernel's folded buffer")
    return flat


class GraphRCNNEngine(CenterPointEngine):
    """``GraphRCNN``: the CenterPoint engine's first stage, its boxes as RoIs, ``gdmae_roi_dfvs_pool``, and the head behind the pooling
    in ``gdmae_roi_graph_forward`` (two launches, bf16 operands in the five wide products, fp32 elsewhere)."""

    def _check_stages(self, model):
        if getattr(model, "point_head", None) is not None:
            _no("a model with a point_head")
        if getattr(model, "roi_head", None) is None:
            _no("a GraphRCNN without a roi_head")

    def _refresh_head(self, dev):
        super()._refresh_head(dev)
        flat = fold_roi_head(self.model.roi_head)
        self.roi_packed = torch.empty(L.load().gdmae_roi_graph_packed_bytes(), dtype=torch.uint8, device=dev)
        L.call("gdmae_roi_graph_pack", L.ptr(flat), L.ptr(self.roi_packed), L.stream())

    def _second_stage(self, points, B, rois, roi_scores, normalized):
        head = self.model.roi_head
        if not (points.is_cuda and rois.is_cuda and roi_scores.is_cuda):
            _no("the second stage runs on device tensors only")
        rois = rois.float().contiguous()
        roi_scores = roi_scores.float().contiguous()
        if rois.dim() != 3 or rois.shape[0] != B or rois.shape[2] < 7 or tuple(roi_scores.shape) != tuple(rois.shape[:2]):
            _no(f"rois {tuple(rois.shape)} / roi_scores {tuple(roi_scores.shape)} (want (B, M, >= 7) and (B, M))")
        M = rois.shape[1]
        dev = rois.device
        r = head.pc_range
        _, num, feats, _ = head.roilocal_dfvs_pool3d_layer.pool(points, rois[..., :7].contiguous(), range_xy=[r[0], r[1], r[3], r[4]])
        if feats.shape[1:] != (256, 11):
            _no(f"pooled features {tuple(feats.shape[1:])} per RoI (the second-stage kernels take 256 points x 11 = 3 + 2 point features + 6)")
        out = {'rcnn_cls': torch.empty(B * M, 1, dtype=torch.float32, device=dev), 'rcnn_reg': torch.empty(B * M, 7, dtype=torch.float32, device=dev),
               'batch_cls_preds': torch.empty(B, M, 1, dtype=torch.float32, device=dev),
               'batch_box_preds': torch.empty(B, M, 7, dtype=torch.float32, device=dev), 'pooled_num': num.view(-1)}
        if B * M:
            ws = torch.empty(L.load().gdmae_roi_graph_workspace_bytes(B * M), dtype=torch.uint8, device=dev)
            L.call("gdmae_roi_graph_forward", L.ptr(feats), L.ptr(num), L.ptr(rois), rois.shape[2], L.ptr(roi_scores), B, M, int(bool(normalized)),
                   L.ptr(self.roi_packed), L.ptr(out['rcnn_cls']), L.ptr(out['rcnn_reg']), L.ptr(out['batch_box_preds']),
                   L.ptr(out['batch_cls_preds']), None, L.ptr(ws), ws.numel(), L.stream())
        return out

    @torch.no_grad()
    def refine(self, batch_dict):
        """The second stage on the caller's RoIs: ``points``, ``batch_size``, ``rois`` (B, M, >= 7), ``roi_scores`` (B, M)
        (probabilities when ``cls_preds_normalized``, logits otherwise), ``roi_labels`` -> rcnn_cls (B M, 1), rcnn_reg (B M, 7),
        batch_cls_preds (B, M, 1), batch_box_preds (B, M, 7), pooled_num (B M).  Rows of padded RoIs (label 0) are computed like any
        other and dropped by ``post_processing``."""
        self._check_fresh()
        with torch.autocast("cuda", enabled=False):
            return self._second_stage(batch_dict['points'], int(batch_dict['batch_size']), batch_dict['rois'], batch_dict['roi_scores'],
                                      batch_dict.get('cls_preds_normalized', False))

    @torch.no_grad()
    def proposals(self, batch_dict):
        """The first stage's RoIs as ``CenterHead.forward`` leaves them: rois (B, M, 7), roi_scores, roi_labels (zero-padded)."""
        maps = self.head_maps(batch_dict)
        B = int(batch_dict['batch_size'])
        hd = self.model.dense_head
        with torch.autocast("cuda", enabled=False):
            rois, scores, labels = hd.reorder_rois_for_refining(B, hd.generate_predicted_boxes(B, maps))
        return {'batch_size': B, 'rois': rois, 'roi_scores': scores, 'roi_labels': labels, 'has_class_labels': True,
                'cls_preds_normalized': True}

    @torch.no_grad()
    def __call__(self, batch_dict):
        bd = self.proposals(batch_dict)
        with torch.autocast("cuda", enabled=False):
            out = self._second_stage(batch_dict['points'], bd['batch_size'], bd['rois'], bd['roi_scores'], True)
            bd['batch_cls_preds'], bd['batch_box_preds'] = out['batch_cls_preds'], out['batch_box_preds']
            if 'gt_boxes' in batch_dict:
                bd['gt_boxes'] = batch_dict['gt_boxes']
            return self.model.post_processing(bd)

    @torch.no_grad()
    def detect(self, batch_dict, recall=None):
        """Both stages on padded device tensors: the first stage through the batched tail, its padded output as the RoIs, then the
        second stage.  ONE host read in between, ``num.max()``: the RoI rows are trimmed to M = max(1, largest count of the batch), the M
        of ``proposals()``, so the second stage runs as many rows as ``engine(batch_dict)`` does and no more.  -> pred_boxes (B, M, 7),
        pred_scores (B, M), pred_labels (B, M) int64 (the RoI labels; 0 in padded rows, whose boxes and scores are zero), num (B).
        ``recall``: as in ``CenterPointEngine.detect``, with the refined boxes as the rcnn side and the RoIs as the roi side (what
        ``post_processing_without_nms`` hands ``generate_recall_record``)."""
        B = int(batch_dict['batch_size'])
        rec = _record(self.model, recall, batch_dict)
        first = super().detect(batch_dict)
        M = max(1, int(first['num'].max()))                       # the host read
        with torch.autocast("cuda", enabled=False):
            rois = first['pred_boxes'][:, :M].contiguous()
            labels = first['pred_labels'][:, :M].contiguous()
            out = self._second_stage(batch_dict['points'], B, rois, first['pred_scores'][:, :M].contiguous(), True)
            real = labels != 0
            boxes, scores = out['batch_box_preds'], out['batch_cls_preds'].max(dim=-1)[0]
            res = {'pred_boxes': torch.where(real.unsqueeze(-1), boxes, torch.zeros_like(boxes)),
                   'pred_scores': torch.where(real, scores, torch.zeros_like(scores)), 'pred_labels': labels, 'num': first['num']}
            if rec is not None:
                rec.update(res['pred_boxes'], res['num'], batch_dict['gt_boxes'], rois=rois, roi_num=first['num'])
            return res


class AnchorEngine(DetectorEngine):
    """``PointPillar`` with ``AnchorHeadSingle``: the three 1 x 1 convolutions, the score threshold and the box decoding of the
    survivors are ``gdmae_anchor_head_infer`` (two launches); the tail of ``post_processing`` runs on the survivors."""

    @staticmethod
    def HEAD():
        from pcdet.models.dense_heads.anchor_head_single import AnchorHeadSingle
        return AnchorHeadSingle

    def _check_post_cfg(self):
        """the branches of ``post_processing`` this engine restates (its messages)"""
        cfg = self.model.model_cfg.POST_PROCESSING
        nms = cfg.NMS_CONFIG
        if nms.MULTI_CLASSES_NMS:
            raise NotImplementedError("MULTI_CLASSES_NMS: True (per-class NMS in post_processing) is not built")
        if not nms.get('NMS', True) or cfg.get('OUTPUT_RAW_SCORE', False) or nms.NMS_TYPE != 'nms_gpu':
            raise NotImplementedError("post_processing: only NMS_TYPE nms_gpu with OUTPUT_RAW_SCORE False is built")
        if cfg.SCORE_THRESH is None:
            _no("SCORE_THRESH: None (the anchor head's selection kernel needs a score threshold)")
        return cfg

    def _refresh_head(self, dev):
        hd, cin = self.model.dense_head, self.bev_out
        self._check_post_cfg()
        if hd.conv_dir_cls is None:
            _no("an anchor head without the direction classifier (USE_DIRECTION_CLASSIFIER)")
        t = hd._device_tables(dev)             # refuses anchor sets with several bottom heights or different strides
        K, C, nb = hd.num_anchors_per_location, hd.num_class, int(hd.model_cfg.NUM_DIR_BINS)
        for conv, n_out in ((hd.conv_cls, K * C), (hd.conv_box, K * 7), (hd.conv_dir_cls, K * nb)):
            if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and
                    conv.groups == 1 and conv.in_channels == cin and conv.out_channels == n_out):
                _no(f"anchor head convolution {conv} (1 x 1, {cin} -> {n_out})")
        if cin % 32 != 0 or cin > 256:
            _no(f"anchor head on a {cin}-channel map (the kernel reads multiples of 32 up to 256)")
        if K * (C + 7 + nb) > 96 or C > 8 or nb > 8:
            _no(f"anchor head too wide for the kernel: {K} anchors x ({C} + 7 + {nb}) = {K * (C + 7 + nb)} columns (96 at most)")
        ws = [c.weight.detach().float().reshape(c.out_channels, cin).contiguous() for c in (hd.conv_cls, hd.conv_box, hd.conv_dir_cls)]
        bs = [None if c.bias is None else c.bias.detach().float().contiguous() for c in (hd.conv_cls, hd.conv_box, hd.conv_dir_cls)]
        self.head_packed = torch.empty(L.load().gdmae_anchor_head_infer_packed_bytes(cin), dtype=torch.uint8, device=dev)
        L.call("gdmae_anchor_head_infer_pack", L.ptr(ws[0]), L.ptr(bs[0]), L.ptr(ws[1]), L.ptr(bs[1]), L.ptr(ws[2]), L.ptr(bs[2]), cin, K, C, nb,
               L.ptr(self.head_packed), L.stream())
        self.tables = t
        self.K, self.C, self.nb, self.cin = K, C, nb, cin
        self.dir_offset, self.dir_limit_offset = float(hd.model_cfg.DIR_OFFSET), float(hd.model_cfg.DIR_LIMIT_OFFSET)

    def _head(self, x2, want_rows):
        """-> (count (B), score (B, A), label (B, A), box (B, A, 7), rows (B H W, K (C + 7 + nb)) fp32 or None); the first count[b]
        entries of a sample are written"""
        B, H, W, c = x2.shape
        t, K, C, nb = self.tables, self.K, self.C, self.nb
        if (H, W) != (t['H'], t['W']) or c != self.cin:
            _no(f"a {H} x {W} x {c} BEV map in front of an anchor head built for {t['H']} x {t['W']} x {self.cin}")
        assert x2.dtype == BF16 and x2.is_contiguous()
        dev, A = x2.device, H * W * K
        thresh = float(self._check_post_cfg().SCORE_THRESH)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        idx = torch.empty(B, A, dtype=torch.int32, device=dev)
        score = torch.empty(B, A, dtype=torch.float32, device=dev)
        label = torch.empty(B, A, dtype=torch.int32, device=dev)
        box = torch.empty(B, A, 7, dtype=torch.float32, device=dev)
        rows = torch.empty(B * H * W, K * (C + 7 + nb), dtype=torch.float32, device=dev) if want_rows else None
        ws = torch.empty(L.load().gdmae_anchor_head_infer_workspace_bytes(B, H, W, K), dtype=torch.uint8, device=dev)
        L.call("gdmae_anchor_head_infer", L.ptr(x2), B, H, W, c, K, C, nb, L.ptr(self.head_packed), L.ptr(t['xc']), L.ptr(t['yc']),
               L.ptr(t['slot']), self.dir_offset, self.dir_limit_offset, thresh, L.ptr(rows), L.ptr(count), L.ptr(idx), L.ptr(score),
               L.ptr(label), L.ptr(box), L.ptr(ws), L.stream())
        return count, score, label, box, rows

    @torch.no_grad()
    def head_maps(self, batch_dict) -> HeadMaps:
        self._check_fresh()
        with torch.autocast("cuda", enabled=False):
            B, x2, sf, pf, vox = self._trunk(batch_dict)
            rows = self._head(x2, True)[4]
        _, H, W, _ = x2.shape
        K, C, nb = self.K, self.C, self.nb
        r = rows.view(B, H, W, -1)
        out = HeadMaps([{'cls_preds': r[..., :K * C], 'box_preds': r[..., K * C:K * (C + 7)], 'dir_cls_preds': r[..., K * (C + 7):]}])
        return self._with_maps(out, x2, sf, pf, vox)

    @torch.no_grad()
    def __call__(self, batch_dict):
        self._check_fresh()
        m = self.model
        with torch.autocast("cuda", enabled=False):
            B, x2, _, _, _ = self._trunk(batch_dict)
            count, score, label, box, _ = self._head(x2, False)
            counts = count.tolist()                     # the one host read of the call: the output shapes depend on it
            bd = {'batch_size': B}
            if 'gt_boxes' in batch_dict:
                bd['gt_boxes'] = batch_dict['gt_boxes']
            recall_dict, pred_dicts = {}, []
            for b in range(B):
                n = counts[b]
                pred, recall_dict = m.finish_sample(box[b, :n], score[b, :n], label[b, :n].long(), recall_dict, b, bd)
                pred_dicts.append(pred)
            return pred_dicts, recall_dict

    @torch.no_grad()
    def detect(self, batch_dict, recall=None):
        """The trunk, the two-launch head, then the batched tail (``Detector3DTemplate.finish_batch``: three launches for all samples):
        pred_boxes (B, n, 7), pred_scores (B, n), pred_labels (B, n) int64, num (B) int32 on the device, rows at or beyond num[b] zero;
        n depends on the config only.  Nothing is read on the host after the trunk;
        ``Detector3DTemplate.padded_to_pred_dicts`` gives the per-sample list of ``engine(batch_dict)``.  ``recall``: as in
        ``CenterPointEngine.detect``."""
        self._check_fresh()
        rec = _record(self.model, recall, batch_dict)
        with torch.autocast("cuda", enabled=False):
            _, x2, _, _, _ = self._trunk(batch_dict)
            count, score, label, box, _ = self._head(x2, False)
            out = self.model.finish_batch(count, score, label, box)
            if rec is not None:
                rec.update(out['pred_boxes'], out['num'], batch_dict['gt_boxes'])
            return out


def compile_detector(model) -> DetectorEngine:
    """Fold and pack ``model`` (a CenterPoint, PointPillar or GraphRCNN from ``pcdet.models.build_network``, in eval mode, on the
    GPU) for inference."""
    from pcdet.models.detectors.centerpoint import CenterPoint
    from pcdet.models.detectors.graph_rcnn import GraphRCNN
    from pcdet.models.detectors.pointpillar import PointPillar
    if isinstance(model, CenterPoint):
        return CenterPointEngine(model)
    if isinstance(model, PointPillar):
        return AnchorEngine(model)
    if isinstance(model, GraphRCNN):
        return GraphRCNNEngine(model)
    _no(f"compile_detector covers the CenterPoint, PointPillar and GraphRCNN detectors, not {type(model).__name__}")
