"""Nystrom attention, restated: the one third-party layer the reference's TransMIL needs (models/model_mil.py:6,
:108-116: `from nystrom_attention import NystromAttention`).

The package (lucidrains/nystrom-attention; the TransMIL authors pin 0.0.9, the reference pins nothing -- it has no
requirements file) is absent from this image and from the reference tree, so the reference's own TransMIL cannot be
constructed here and NO fixture can be generated for it: **parity of this module is unpinned**.  What follows is the
published algorithm (Xiong et al., "Nystromformer", AAAI 2021, as that package implements it): segment-mean landmarks,
three softmax kernels, the Moore-Penrose pseudo-inverse by the cubic iteration of the paper, the depth-wise
convolution residual on the values.  Module / parameter names follow the package (`to_qkv`, `to_out.0`, `res_conv`)
so that a TransMIL checkpoint trained with it loads.  Checked here against what CAN be checked: exact softmax
attention in the limit where every token is its own landmark, the pseudo-inverse against `torch.linalg.pinv`, shapes
and padding (tests/test_baselines_cpu.py).  Plain torch operations: this is a signature shim (SURVEY.md section 8,
f3); with `fused = True` the no-grad forward runs on the kernels of csrc/moc_nystrom.hip instead, which are checked
against THIS restatement (tests/test_gpu_nystrom.py) and pin nothing more than it does; `fused_pinv = True` on top of it
takes the pseudo-inverse from csrc/moc_nystrom_pinv.hip, checked against moore_penrose_iter_pinv below
(tests/test_gpu_nystrom_pinv.py); `fused_train = True` on top of `fused` lets the passes that want a gradient run on the same
two products too, through LandmarkValues / TokenValues below, whose backward is csrc/moc_nystrom_bwd.hip, checked against
float64 autograd of THIS restatement (tests/test_gpu_nystrom_train.py); `fused_conv = True` on top of both keeps kernel B's
residual convolution in those passes too, through TokenValuesResidual, whose backward adds csrc/moc_nystrom_conv_bwd.hip
(the convolution's value and tap gradients), checked the same way (tests/test_gpu_nystrom_conv.py);
`fused_pinv_train = True` on top of `fused` and `fused_train` takes the pseudo-inverse of those passes from LandmarkPinv, whose
forward is moc_nystrom_pinv_iterates and whose backward is moc_nystrom_pinv_backward (csrc/moc_nystrom_pinv.hip), checked
against float64 autograd of moore_penrose_iter_pinv (tests/test_gpu_nystrom_pinv_bwd.py).  `forward_rows(x, rows)` is the
layer's answer to "where does this token look": the forward's result and the wanted rows of attn1 @ pinv @ attn3, on
csrc/moc_nystrom_rows.hip where `fused` applies and on torch elsewhere, checked against a float64 evaluation of the whole
matrix (tests/test_nystrom_rows_cpu.py, tests/test_gpu_nystrom_rows.py)."""
from __future__ import annotations

from math import ceil

import torch
import torch.nn as nn
import torch.nn.functional as F


def moore_penrose_iter_pinv(x: torch.Tensor, iters: int = 6) -> torch.Tensor:
    """Pseudo-inverse of the [..., m, m] landmark kernel by Z <- 1/4 Z (13 I - XZ (15 I - XZ (7 I - XZ)))."""
    abs_x = x.abs()
    col, row = abs_x.sum(dim=-1), abs_x.sum(dim=-2)
    z = x.transpose(-1, -2) / (col.max() * row.max())
    eye = torch.eye(x.shape[-1], device=x.device, dtype=x.dtype).unsqueeze(0)
    for _ in range(iters):
        xz = x @ z
        z = 0.25 * z @ (13 * eye - (xz @ (15 * eye - (xz @ (7 * eye - xz)))))
    return z


class LandmarkValues(torch.autograd.Function):
    """W = softmax_over_tokens(q_l k^T) v per head on kernel A, from qkv [n_pad, 1536] and the scaled landmark queries q_l
    [8, 256, 64]; the forward keeps the per-landmark log-sum-exp, from which the backward (moc_nystrom_landmark_backward)
    recomputes the weights tile by tile.  The qkv gradient has dk and dv and zeros in the q columns."""

    @staticmethod
    def forward(ctx, qkv, q_l):
        from . import engine
        W, lse = engine.nystrom_landmark_values_lse(qkv, q_l)
        ctx.save_for_backward(qkv, q_l, W, lse)
        return W

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dW):
        from . import engine
        qkv, q_l, W, lse = ctx.saved_tensors
        return engine.nystrom_landmark_backward(qkv, q_l, W, lse, dW)


class TokenValues(torch.autograd.Function):
    """out = softmax_256(scale q k_l^T) Y per head and token on kernel B WITHOUT its residual convolution, [n_pad, 512];
    the backward (moc_nystrom_token_backward) recomputes the weights.  The qkv gradient has dq and zeros in the k and v
    columns."""

    @staticmethod
    def forward(ctx, qkv, k_l, Y, scale):
        from . import engine
        ctx.save_for_backward(qkv, k_l, Y)
        ctx.scale = scale
        return engine.nystrom_token_values(qkv, k_l, Y, None, scale)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        from . import engine
        qkv, k_l, Y = ctx.saved_tensors
        dqkv, dk_l, dY = engine.nystrom_token_backward(qkv, k_l, Y, ctx.scale, dout)
        return dqkv, dk_l, dY, None


class TokenValuesResidual(torch.autograd.Function):
    """TokenValues WITH kernel B's residual convolution of v by conv_w [8, taps]: the forward is bit for bit what the no-grad
    fused forward computes; the backward is moc_nystrom_token_backward, then moc_nystrom_conv_backward on the same qkv
    gradient, which leaves dq in the q columns, zeros in the k columns and the convolution's dv in the v columns."""

    @staticmethod
    def forward(ctx, qkv, k_l, Y, conv_w, scale):
        from . import engine
        ctx.save_for_backward(qkv, k_l, Y, conv_w)
        ctx.scale = scale
        return engine.nystrom_token_values(qkv, k_l, Y, conv_w, scale)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        from . import engine
        qkv, k_l, Y, conv_w = ctx.saved_tensors
        dqkv, dk_l, dY = engine.nystrom_token_backward(qkv, k_l, Y, ctx.scale, dout)
        dconv_w = engine.nystrom_conv_backward(qkv, conv_w, dout, dqkv)
        return dqkv, dk_l, dY, dconv_w, None


class LandmarkPinv(torch.autograd.Function):
    """moore_penrose_iter_pinv of attn2 [8, 256, 256] on moc_nystrom_pinv_iterates: the forward keeps attn2 and the
    iters + 1 iterates ((iters + 1) x 2 MiB) and returns the last, bit for bit engine.nystrom_pinv's result; the backward
    (moc_nystrom_pinv_backward) recomputes XZ, P2 and P3 of every iteration from them."""

    @staticmethod
    def forward(ctx, attn2, iters):
        from . import engine
        Zs = engine.nystrom_pinv_iterates(attn2, iters)
        ctx.save_for_backward(attn2, Zs)
        ctx.iters = iters
        return Zs[iters]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dZ):
        from . import engine
        attn2, Zs = ctx.saved_tensors
        return engine.nystrom_pinv_backward(attn2, Zs, dZ, ctx.iters), None


class NystromAttention(nn.Module):
    def __init__(self, dim, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6, residual=True,
                 residual_conv_kernel=33, eps=1e-8, dropout=0.0):
        super().__init__()
        self.eps, self.heads = eps, heads
        inner = heads * dim_head
        self.num_landmarks, self.pinv_iterations = num_landmarks, pinv_iterations
        self.scale = dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, inner * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(dropout))
        self.residual = residual
        if residual:
            k = residual_conv_kernel
            self.res_conv = nn.Conv2d(heads, heads, (k, 1), padding=(k // 2, 0), groups=heads, bias=False)

    # True: forward takes forward_fused (the HIP kernels of moc_nystrom.hip wherever they apply, this torch code elsewhere)
    fused = False
    # True: forward_fused, where its kernels apply, takes the pseudo-inverse from engine.nystrom_pinv (moc_nystrom_pinv.hip)
    # instead of moore_penrose_iter_pinv; no effect on any call that runs the torch code
    fused_pinv = False
    # True: forward_fused, where its kernels apply but for a wanted gradient, keeps the two products on the kernels and
    # takes their gradient from moc_nystrom_bwd.hip (_forward_fused_train); no effect without `fused`, nor under no_grad
    fused_train = False
    # True: _forward_fused_train, for a layer with a residual, keeps the residual convolution inside kernel B and takes its two
    # gradients from moc_nystrom_conv_bwd.hip (TokenValuesResidual); no effect on any call that does not run _forward_fused_train
    fused_conv = False
    # True: _forward_fused_train takes the pseudo-inverse and its gradient from moc_nystrom_pinv.hip (LandmarkPinv) instead of
    # moore_penrose_iter_pinv under autograd; no effect on any call that does not run _forward_fused_train
    fused_pinv_train = False

    def forward(self, x, mask=None, return_attn=False):
        if self.fused:
            return self.forward_fused(x, mask=mask, return_attn=return_attn)
        return self._forward_torch(x, mask=mask, return_attn=return_attn)

    def _wants_grad(self, x) -> bool:
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _fused_applies(self, x, mask, return_attn) -> bool:
        return not self._wants_grad(x) and self._kernels_apply(x, mask, return_attn)   # the forward kernels form no gradient

    def _kernels_apply(self, x, mask, return_attn) -> bool:
        if mask is not None or return_attn:
            return False
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] == 1 and x.shape[1] >= 1
                and x.is_contiguous()):
            return False
        if not (self.heads == 8 and self.to_qkv.out_features == 3 * 8 * 64 and self.num_landmarks == 256
                and all(p.dtype == torch.float32 and p.is_cuda for p in self.parameters())):
            return False
        return not self.residual or tuple(self.res_conv.kernel_size) == (33, 1)

    def forward_fused(self, x, mask=None, return_attn=False):
        """The no-grad forward on the HIP kernels: to_qkv, the landmark means, attn2 and its
        pseudo-inverse in torch (the pseudo-inverse on moc_nystrom_pinv with `fused_pinv`); W = softmax(q_l k^T) v (kernel A); Y = pinv W; softmax(q k_l^T) Y + res_conv(v) (kernel
        B); to_out.  Neither [8, n, 256] score matrix is formed.  Wherever the kernels do not apply -- a gradient is
        wanted, x is not a contiguous fp32 [1, n, dim] CUDA tensor, another layer shape, mask / return_attn -- this is
        the torch code above, bit for bit; with `fused_train`, a call that fails ONLY for the wanted gradient is
        _forward_fused_train."""
        if self.fused_train and self._wants_grad(x) and self._kernels_apply(x, mask, return_attn):
            return self._forward_fused_train(x)
        if not self._fused_applies(x, mask, return_attn):
            return self._forward_torch(x, mask=mask, return_attn=return_attn)
        from . import engine
        n, h, m = x.shape[1], self.heads, self.num_landmarks
        if n % m > 0:
            x = F.pad(x, (0, 0, m - (n % m), 0), value=0)
        qkv = self.to_qkv(x)[0]                           # [n_pad, 1536]: q | k | v, each head-major in its 512 columns
        l, inner = qkv.shape[0] // m, qkv.shape[1] // 3
        # the landmark means of q and k in one pass over their 1,024 columns; the scale (64 ** -0.5, a power of two) commutes
        # with the sum and the division exactly, so it is applied to the [256, 512] means and not to the [n, 512] queries
        means = qkv[:, :2 * inner].reshape(m, l, 2 * inner).sum(dim=1) / l
        q_l = (means[:, :inner] * self.scale).reshape(m, h, -1).transpose(0, 1).contiguous()                        # h m d
        k_l = means[:, inner:].reshape(m, h, -1).transpose(0, 1).contiguous()
        attn2 = (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1)
        if self.fused_pinv:
            pinv = engine.nystrom_pinv(attn2, self.pinv_iterations)
        else:
            pinv = moore_penrose_iter_pinv(attn2.unsqueeze(0), self.pinv_iterations)[0]
        W =engine.nystrom_landmark_values(qkv, q_l)      # softmax over the tokens of q_l k^T, times v
        conv_w = self.res_conv.weight.reshape(h, -1) if self.residual else None
        out = engine.nystrom_token_values(qkv, k_l, pinv @ W, conv_w, self.scale)
        return self.to_out(out.unsqueeze(0))[:, -n:]

    def _forward_fused_train(self, x):
        """forward_fused's dataflow with autograd kept ("training"): to_qkv, the landmark means, attn2
        and its pseudo-inverse are tracked torch operations; W = LandmarkValues(qkv, q_l); Y = pinv W in torch;
        TokenValues(qkv, k_l, Y) without the residual; then res_conv(v), to_out and the slice in torch.  Neither [8, n, 256]
        score matrix is formed or kept: both backward kernels recompute their weights.  The pseudo-inverse is
        moore_penrose_iter_pinv here -- `fused_pinv` is ignored, its entry forms no gradient -- unless `fused_pinv_train` is set:
        then it is LandmarkPinv, the same kernels with the iterates kept and a backward of their own.  The residual
        convolution and its two gradients stay on torch, unless `fused_conv` is set: then the residual is kernel B's own
        (TokenValuesResidual) and res_conv's forward is not called."""
        n, h, m = x.shape[1], self.heads, self.num_landmarks
        if n % m > 0:
            x = F.pad(x, (0, 0, m - (n % m), 0), value=0)
        qkv = self.to_qkv(x)[0]                           # [n_pad, 1536]
        n_pad, inner = qkv.shape[0], qkv.shape[1] // 3
        means = qkv[:, :2 * inner].reshape(m, n_pad // m, 2 * inner).sum(dim=1) / (n_pad // m)
        q_l = (means[:, :inner] * self.scale).reshape(m, h, -1).transpose(0, 1).contiguous()                        # h m d
        k_l = means[:, inner:].reshape(m, h, -1).transpose(0, 1).contiguous()
        attn2 = (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1)
        if self.fused_pinv_train:
            pinv = LandmarkPinv.apply(attn2, self.pinv_iterations)
        else:
            pinv = moore_penrose_iter_pinv(attn2.unsqueeze(0), self.pinv_iterations)[0]
        W = LandmarkValues.apply(qkv, q_l)
        if self.residual and self.fused_conv:                                         # (the reshape stays tracked)
            out = TokenValuesResidual.apply(qkv, k_l, pinv @ W, self.res_conv.weight.reshape(h, -1), self.scale)
        else:
            out = TokenValues.apply(qkv, k_l, pinv @ W, self.scale)                   # [n_pad, 512]
            if self.residual:
                v = qkv[:, 2 * inner:].reshape(1, n_pad, h, -1).transpose(1, 2)     # [1, 8, n_pad, 64], a view
                out = out + self.res_conv(v).transpose(1, 2).reshape(n_pad, inner)
        return self.to_out(out.unsqueeze(0))[:, -n:]

    def forward_rows(self, x, rows):
        """(out, attn) under no_grad: `out` is bit for bit what forward(x) returns under no_grad for the same module state,
        `attn` [heads, len(rows), n] ([b, heads, len(rows), n] for a batch) the wanted rows of the layer's attention matrix
        attn1 @ pinv @ attn3, columns restricted to the last n (the real tokens) and not renormalised.  `rows`: one or more
        indices into the unpadded sequence, 0 <= r < n.  Neither result carries a gradient.

        What a row is: a Nystrom row is an approximation of softmax(scale q k^T)'s.  It can be slightly negative (the
        pseudo-inverse has entries of either sign).  Over all n_pad columns it sums to coef.sum(), coef = attn1[row] @ pinv,
        about 1, because each row of attn3 sums to one; the front padding's zero keys take their share of that: a random
        37-token sequence padded to 48 leaves 0.77 on the real tokens.  The residual convolution, which adds values without
        any weights, is not part of it.

        With `fused`, where forward_fused's kernels apply (_kernels_apply) and for at most 16 rows, the forward is
        forward_fused's own (kernel A through engine.nystrom_landmark_values_lse, whose W is bit for bit the other entry's;
        `fused_pinv` honoured), coef [8, R, 256] comes from the rows' own q in torch, and the rows from
        engine.nystrom_attention_rows (csrc/moc_nystrom_rows.hip), one pass over the keys that reuses kernel A's
        log-sum-exp: attn3, the [8, 256, n_pad] score matrix, is not formed.  Everywhere else -- the CPU, another layer
        shape, more rows, a batch -- the same quantities come from torch for the wanted rows only, attn1[rows] @ pinv @
        attn3, which forms attn3."""
        with torch.no_grad():
            n = x.shape[1]
            rows = [int(r) for r in (rows.reshape(-1).tolist() if torch.is_tensor(rows) else rows)]
            if len(rows) < 1 or min(rows) < 0 or max(rows) >= n:
                raise ValueError(f"forward_rows: rows must be one or more indices in 0..{n - 1}, got {rows}")
            idx = torch.tensor(rows, dtype=torch.long, device=x.device)
            kernels = self.fused and self._kernels_apply(x, None, False)
            if kernels and idx.numel() <= 16:
                return self._rows_fused(x, idx)
            out, attn = self._rows_torch(x, idx)
            if kernels:                                   # more than 16 rows: the rows from torch, forward's own bits in `out`
                out = self.forward_fused(x)
            return out, attn

    def _rows_fused(self, x, idx):
        """forward_fused's dataflow with kernel A's log-sum-exp kept, then the rows (forward_rows)."""
        from . import engine
        n, h, m = x.shape[1], self.heads, self.num_landmarks
        if n % m > 0:
            x = F.pad(x, (0, 0, m - (n % m), 0), value=0)
        qkv = self.to_qkv(x)[0]                           # [n_pad, 1536]
        l, inner = qkv.shape[0] // m, qkv.shape[1] // 3
        means = qkv[:, :2 * inner].reshape(m, l, 2 * inner).sum(dim=1) / l
        q_l = (means[:, :inner] * self.scale).reshape(m, h, -1).transpose(0, 1).contiguous()                        # h m d
        k_l = means[:, inner:].reshape(m, h, -1).transpose(0, 1).contiguous()
        attn2 = (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1)
        if self.fused_pinv:
            pinv = engine.nystrom_pinv(attn2, self.pinv_iterations)
        else:
            pinv = moore_penrose_iter_pinv(attn2.unsqueeze(0), self.pinv_iterations)[0]
        W, lse = engine.nystrom_landmark_values_lse(qkv, q_l)
        conv_w = self.res_conv.weight.reshape(h, -1) if self.residual else None
        out = engine.nystrom_token_values(qkv, k_l, pinv @ W, conv_w, self.scale)
        q_r = qkv[idx + (qkv.shape[0] - n), :inner].reshape(idx.numel(), h, -1).transpose(0, 1) * self.scale       # h R d
        coef = (q_r @ k_l.transpose(-1, -2)).softmax(dim=-1) @ pinv                                                # h R m
        attn = engine.nystrom_attention_rows(qkv, q_l, lse, coef)
        return self.to_out(out.unsqueeze(0))[:, -n:], attn[..., -n:]

    def _rows_torch(self, x, idx):
        """_forward_torch's dataflow, operation for operation (`out` has its bits), and attn1[rows] @ pinv @ attn3."""
        b, n, _ = x.shape
        h, m = self.heads, self.num_landmarks
        if n % m > 0:
            x = F.pad(x, (0, 0, m - (n % m), 0), value=0)
        q, k, v = self.to_qkv(x).chunk(3, dim=-1)
        q, k, v = (t.reshape(b, t.shape[1], h, -1).transpose(1, 2) for t in (q, k, v))      # b h n d
        q = q * self.scale
        l = ceil(n / m)
        q_l = q.reshape(b, h, -1, l, q.shape[-1]).sum(dim=3) / l
        k_l = k.reshape(b, h, -1, l, k.shape[-1]).sum(dim=3) / l
        attn1 = (q @ k_l.transpose(-1, -2)).softmax(dim=-1)
        attn2 = (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1)
        attn3 = (q_l @ k.transpose(-1, -2)).softmax(dim=-1)
        pinv = moore_penrose_iter_pinv(attn2, self.pinv_iterations)
        out = (attn1 @ pinv) @ (attn3 @ v)
        if self.residual:
            out = out + self.res_conv(v)
        out = out.transpose(1, 2).reshape(b, out.shape[2], -1)
        attn = ((attn1[:, :, idx + (attn1.shape[2] - n)] @ pinv) @ attn3)[..., -n:]          # b h R n
        return self.to_out(out)[:, -n:], attn[0] if b == 1 else attn

    def _forward_torch(self, x, mask=None, return_attn=False):
        assert mask is None and not return_attn, "the reference calls attn(x) only (models/model_mil.py:119)"
        b, n, _ = x.shape
        h, m = self.heads, self.num_landmarks
        if n % m > 0:                                     # pad at the FRONT so that the length divides into m landmarks
            x = F.pad(x, (0, 0, m - (n % m), 0), value=0)
        q, k, v = self.to_qkv(x).chunk(3, dim=-1)
        q, k, v = (t.reshape(b, t.shape[1], h, -1).transpose(1, 2) for t in (q, k, v))      # b h n d
        q = q * self.scale
        l = ceil(n / m)                                   # tokens per landmark
        q_l = q.reshape(b, h, -1, l, q.shape[-1]).sum(dim=3) / l
        k_l = k.reshape(b, h, -1, l, k.shape[-1]).sum(dim=3) / l
        attn1 = (q @ k_l.transpose(-1, -2)).softmax(dim=-1)
        attn2 = (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1)
        attn3 = (q_l @ k.transpose(-1, -2)).softmax(dim=-1)
        out = (attn1 @ moore_penrose_iter_pinv(attn2, self.pinv_iterations)) @ (attn3 @ v)
        if self.residual:
            out = out + self.res_conv(v)
        out = out.transpose(1, 2).reshape(b, out.shape[2], -1)
        return self.to_out(out)[:, -n:]
