"""Max-instance MIL baselines under the reference's names and forward contract (SURVEY.md section 8,
row f3; reference models/model_mil.py).  forward(h) -> (top_instance logits [1, C], Y_prob [1, C],
Y_hat, y_probs [N, C], results_dict).  The per-instance classifier is torch (a plain library GEMM);
picking the top instance over the N patches runs on the HIP path (pool_autograd) and autograd flows
through the picked row only, as in the reference.  Parameter names match (`classifier.{0,2}` /
`fc.0`, `classifiers.{c}`), so reference checkpoints load.  TransMIL (plain torch + the restated Nystrom attention of
moc_amd/nystrom.py; parity unpinned: the reference's own class cannot be built without the absent third-party
package) keeps the contract (logits, Y_prob, Y_hat, None, None); its switches `fused`, `fused_pinv`, `fused_train`, `fused_conv`
and `fused_pinv_train` (all off by default) put its two attention layers on the HIP kernels of moc_nystrom*.hip -- the no-grad passes, their
pseudo-inverse, and the passes that want a gradient; `fused_ppeg` (off by default, a switch of its own) puts `pos_layer` on
moc_ppeg.hip.  `TransMIL.attention_maps(data)` returns forward's logits and the class token's attention over the bag's
patches in either layer, under the same switches (with `fused`, the rows come from moc_nystrom_rows.hip)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .pool_autograd import top_entry, top_rows


def _plain(m):
    return getattr(m, "module", m)            # the reference indexes `.module` (DataParallel) in one branch


class MIL_fc(nn.Module):
    """Binary max-instance MIL (models/model_mil.py:11-51)."""

    size_dict = {"small": [1024, 512], "benchmark": [384, 512]}

    def __init__(self, gate=True, size_arg="benchmark", dropout=False, n_classes=2, top_k=1):
        super().__init__()
        assert n_classes == 2
        d_in, d_hid = self.size_dict[size_arg]
        layers = [nn.Linear(d_in, d_hid), nn.ReLU()]
        if dropout:
            layers.append(nn.Dropout(0.25))
        layers.append(nn.Linear(d_hid, n_classes))
        self.classifier = nn.Sequential(*layers)
        self.top_k = top_k

    def relocate(self):
        self.classifier.to(torch.device("cuda"))

    def forward(self, h, return_features=False):
        net = _plain(self.classifier)
        if return_features:
            h = net[:-1](h)
            logits = net[-1](h)
        else:
            logits = net(h)                                   # [N, 2]
        y_probs = F.softmax(logits, dim=1)
        pick = top_rows(y_probs[:, 1], self.top_k).view(1,)   # top_k == 1 in every caller (:40)
        top_instance = torch.index_select(logits, 0, pick)
        Y_hat = torch.topk(top_instance, 1, dim=1)[1]
        Y_prob = F.softmax(top_instance, dim=1)
        results = {}
        if return_features:
            results["features"] = torch.index_select(h, 0, pick)
        return top_instance, Y_prob, Y_hat, y_probs, results


class MIL_fc_mc(nn.Module):
    """Multi-class max-instance MIL: one 1-logit head per class, the instance holding the single
    largest class probability represents the bag (models/model_mil.py:54-101)."""

    size_dict = {"small": [1024, 512]}

    def __init__(self, gate=True, size_arg="small", dropout=False, n_classes=2, top_k=1):
        super().__init__()
        assert n_classes > 2
        d_in, d_hid = self.size_dict[size_arg]
        layers = [nn.Linear(d_in, d_hid), nn.ReLU()]
        if dropout:
            layers.append(nn.Dropout(0.25))
        self.fc = nn.Sequential(*layers)
        self.classifiers = nn.ModuleList([nn.Linear(d_hid, 1) for _ in range(n_classes)])
        self.top_k, self.n_classes = top_k, n_classes
        assert self.top_k == 1

    def relocate(self):
        dev = torch.device("cuda")
        self.fc, self.classifiers = self.fc.to(dev), self.classifiers.to(dev)

    def forward(self, h, return_features=False):
        h = self.fc(h)
        heads = _plain(self.classifiers)
        logits = torch.cat([heads[c](h) for c in range(self.n_classes)], dim=1)      # [N, C]
        y_probs = F.softmax(logits, dim=1)
        row, cls = top_entry(y_probs)
        pick = torch.tensor([row], device=h.device)
        top_instance = logits[pick]
        Y_hat = torch.tensor([cls], device=h.device)
        Y_prob = y_probs[pick]
        results = {}
        if return_features:
            results["features"] = torch.index_select(h, 0, pick)
        return top_instance, Y_prob, Y_hat, y_probs, results


class TransLayer(nn.Module):
    """models/model_mil.py:105-122."""

    def __init__(self, norm_layer=nn.LayerNorm, dim=512):
        super().__init__()
        from .nystrom import NystromAttention
        self.norm = norm_layer(dim)
        self.attn = NystromAttention(dim=dim, dim_head=dim // 8, heads=8, num_landmarks=dim // 2, pinv_iterations=6,
                                     residual=True, dropout=0.1)

    def forward(self, x):
        return x + self.attn(self.norm(x))

    def forward_rows(self, x, rows):
        """(forward(x), the wanted rows of the attention matrix) without a gradient: NystromAttention.forward_rows."""
        out, attn = self.attn.forward_rows(self.norm(x), rows)
        return x + out, attn


class PPEGFused(torch.autograd.Function):
    """PPEG on moc_ppeg.hip for passes that want a gradient: the forward is engine.ppeg_forward's launch, bit for bit the
    no-grad pass; it keeps x and the three weights, and the backward is engine.ppeg_backward (one 49-tap pass over dout
    with the table read backwards, and 50 sums per channel)."""

    @staticmethod
    def forward(ctx, x, H, W, w7, b7, w5, b5, w3, b3):
        from . import engine
        ctx.save_for_backward(x, w7, w5, w3)
        ctx.hw = (H, W)
        return engine.ppeg_forward(x, H, W, w7, b7, w5, b5, w3, b3)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        from . import engine
        x, w7, w5, w3 = ctx.saved_tensors
        dx, dw7, db7, dw5, db5, dw3, db3 = engine.ppeg_backward(x, ctx.hw[0], ctx.hw[1], w7, w5, w3, dout)
        return dx, None, None, dw7, db7, dw5, db5, dw3, db3


class PPEG(nn.Module):
    """models/model_mil.py:125-139: depth-wise 7 / 5 / 3 convolutions over the patch tokens laid out as a square.
    `fused = True` (off by default) takes the whole module -- the three convolutions, the identity, the biases and the
    class-token row -- from moc_ppeg.hip where `_fusable` holds, with and without a gradient; everything else is the
    torch code below, bit for bit."""

    fused = False

    def __init__(self, dim=512):
        super().__init__()
        self.proj = nn.Conv2d(dim, dim, 7, 1, 7 // 2, groups=dim)
        self.proj1 = nn.Conv2d(dim, dim, 5, 1, 5 // 2, groups=dim)
        self.proj2 = nn.Conv2d(dim, dim, 3, 1, 3 // 2, groups=dim)

    def _fusable(self, x, H, W) -> bool:
        """x a contiguous fp32 CUDA [1, 1 + H W, 512]; all six parameters fp32 CUDA; the three convolutions as built."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] == 1 and x.shape[2] == 512
                and H >= 1 and W >= 1 and x.shape[1] == 1 + H * W and H * W <= (1 << 22) and x.is_contiguous()):
            return False
        for conv, k in ((self.proj, 7), (self.proj1, 5), (self.proj2, 3)):
            if not (conv.kernel_size == (k, k) and conv.padding == (k // 2, k // 2) and conv.groups == 512
                    and conv.stride == (1, 1) and conv.dilation == (1, 1) and conv.padding_mode == "zeros"
                    and conv.bias is not None and conv.weight.shape == (512, 1, k, k)):
                return False
            for p in (conv.weight, conv.bias):
                if not (p.is_cuda and p.dtype == torch.float32):
                    return False
        return True

    def forward(self, x, H, W):
        if self.fused and self._fusable(x, H, W):
            params = (self.proj.weight, self.proj.bias, self.proj1.weight, self.proj1.bias, self.proj2.weight, self.proj2.bias)
            if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
                return PPEGFused.apply(x, H, W, *params)
            from . import engine
            return engine.ppeg_forward(x, H, W, *params)
        B, _, C = x.shape
        cls_token, feat_token = x[:, 0], x[:, 1:]
        cnn_feat = feat_token.transpose(1, 2).view(B, C, H, W)
        x = self.proj(cnn_feat) + cnn_feat + self.proj1(cnn_feat) + self.proj2(cnn_feat)
        x = x.flatten(2).transpose(1, 2)
        return torch.cat((cls_token.unsqueeze(1), x), dim=1)


class TransMIL(nn.Module):
    """models/model_mil.py:142-273: forward(data) -> (logits [B, C], Y_prob, Y_hat, None, None), same modules and
    parameter names (`pos_layer`, `_fc1`, `cls_token`, `layer1`, `layer2`, `norm`, `_fc2`).  Its attention is the
    third-party `nystrom_attention` package, absent here AND in the reference tree (the reference's own import fails in
    this image): the layer is restated in moc_amd/nystrom.py from the published algorithm, and since no reference
    output can be produced, **parity of this class is unpinned** (checked: shapes, the 5-tuple, the padding rule, the
    attention's exact-softmax limit; not checked: a reference number).  Plain torch: a signature shim, row f3."""

    size_dict = {"small": 1024, "big": 1024, "benchmark": 384, "conch": 512, "gigapath": 1536, "virchow": 2560}

    def __init__(self, n_classes, size_arg="small", **kwargs):
        super().__init__()
        size = self.size_dict[size_arg]
        self.pos_layer = PPEG(dim=512)
        self._fc1 = nn.Sequential(nn.Linear(size, 512), nn.ReLU())
        self.cls_token = nn.Parameter(torch.randn(1, 1, 512))
        self.n_classes = n_classes
        self.layer1 = TransLayer(dim=512)
        self.layer2 = TransLayer(dim=512)
        self.norm = nn.LayerNorm(512)
        self._fc2 = nn.Linear(512, self.n_classes)

    @property
    def fused(self) -> bool:
        """Both layers' attention on the fused Nystrom forward (nystrom.NystromAttention.forward_fused) in no-grad passes."""
        return bool(self.layer1.attn.fused and self.layer2.attn.fused)

    @fused.setter
    def fused(self, on: bool):
        self.layer1.attn.fused = self.layer2.attn.fused = bool(on)

    @property
    def fused_pinv(self) -> bool:
        """Both layers' pseudo-inverse on moc_nystrom_pinv (nystrom.NystromAttention.fused_pinv); acts only where `fused` does."""
        return bool(self.layer1.attn.fused_pinv and self.layer2.attn.fused_pinv)

    @fused_pinv.setter
    def fused_pinv(self, on: bool):
        self.layer1.attn.fused_pinv = self.layer2.attn.fused_pinv = bool(on)

    @property
    def fused_train(self) -> bool:
        """Both layers' attention on the fused products in passes that want a gradient too, with the backward of
        moc_nystrom_bwd.hip (nystrom.NystromAttention.fused_train); acts only together with `fused`."""
        return bool(self.layer1.attn.fused_train and self.layer2.attn.fused_train)

    @fused_train.setter
    def fused_train(self, on: bool):
        self.layer1.attn.fused_train = self.layer2.attn.fused_train = bool(on)

    @property
    def fused_conv(self) -> bool:
        """Both layers' residual convolution inside kernel B in passes that want a gradient, with its two gradients from
        moc_nystrom_conv_bwd.hip (nystrom.NystromAttention.fused_conv); acts only together with `fused` and `fused_train`."""
        return bool(self.layer1.attn.fused_conv and self.layer2.attn.fused_conv)

    @fused_conv.setter
    def fused_conv(self, on: bool):
        self.layer1.attn.fused_conv = self.layer2.attn.fused_conv = bool(on)

    @property
    def fused_pinv_train(self) -> bool:
        """Both layers' pseudo-inverse and its gradient on moc_nystrom_pinv.hip in passes that want a gradient
        (nystrom.NystromAttention.fused_pinv_train); acts only together with `fused` and `fused_train`."""
        return bool(self.layer1.attn.fused_pinv_train and self.layer2.attn.fused_pinv_train)

    @fused_pinv_train.setter
    def fused_pinv_train(self, on: bool):
        self.layer1.attn.fused_pinv_train = self.layer2.attn.fused_pinv_train = bool(on)

    @property
    def fused_ppeg(self) -> bool:
        """`pos_layer` on moc_ppeg.hip (PPEG.fused), with and without a gradient: a switch of its own, which needs none of
        the attention switches and changes none of them."""
        return bool(self.pos_layer.fused)

    @fused_ppeg.setter
    def fused_ppeg(self, on: bool):
        self.pos_layer.fused = bool(on)

    def _embed(self, data):
        """fc1, wrap-around padding to a square, class token: (tokens [B, 1 + side^2, 512], side, n)."""
        if len(data.shape) == 2:
            data = data.unsqueeze(0)
        h = self._fc1(data.float())                                       # [B, n, 512]
        H = h.shape[1]
        side = int(np.ceil(np.sqrt(H)))
        h = torch.cat([h, h[:, :side * side - H, :]], dim=1)              # pad with the first rows again
        h = torch.cat((self.cls_token.expand(h.shape[0], -1, -1).to(h.device), h), dim=1)
        return h, side, data.shape[1]

    def _tokens(self, data):
        """_embed, layer 1, PPEG, layer 2 (:236-266)."""
        h, side, n = self._embed(data)
        h = self.layer1(h)
        h = self.pos_layer(h, side, side)
        return self.layer2(h), n

    def attention_maps(self, data):
        """(logits, {"layer1": [8, n], "layer2": [8, n]}) under no_grad: _tokens' walk with each layer's attention asked
        for the class token's row too (TransLayer.forward_rows), then forward's head.  `logits` is bit for bit
        forward(data)[0] under no_grad in eval() with the same switches; a map is the class token's row of that layer's
        Nystrom attention per head over the bag's n patches -- the class token's own column and the wrap-around rows that
        square the bag are dropped -- as NystromAttention.forward_rows describes it: an approximation, not renormalised,
        slightly negative in places.  All six switches keep their meaning; with `fused` the rows come from
        moc_nystrom_rows.hip.  A batch of B bags gives [B, 8, n] maps."""
        with torch.no_grad():
            h, side, n = self._embed(data)
            h, a1 = self.layer1.forward_rows(h, [0])
            h = self.pos_layer(h, side, side)
            h, a2 = self.layer2.forward_rows(h, [0])
            logits = self._fc2(self.norm(h)[:, 0])
            return logits, {"layer1": a1[..., 0, 1:n + 1], "layer2": a2[..., 0, 1:n + 1]}

    def forward_patch_level(self, data):
        h, n = self._tokens(data)
        return self._fc2(h).squeeze(0)[1:n + 1]                           # [n, n_classes], no final norm (:198-200)

    def forward(self, data, **kwargs):
        h, _ = self._tokens(data)
        logits = self._fc2(self.norm(h)[:, 0])                            # [B, n_classes]
        return logits, F.softmax(logits, dim=1), torch.argmax(logits, dim=1), None, None
