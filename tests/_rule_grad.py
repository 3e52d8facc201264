"""Rule-level gradient probes for eqxvision_amd/grad.py (tests/test_rule_grad_host.py, tests/test_rule_grad_gpu.py).

A probe is a tiny `Module` built from the library's own layers whose `__call__` runs a `body(be, L, x, key)`: a composition written
once against a small backend interface.  `Hip` is the library (the hooked `ops.*` entries, `layers.SqueezeExcitation`,
`nn.Dropout`, `layers.DropPath`), `Twin` restates every entry with plain torch in float64 (the reference: `torch.autograd.grad`) or
float32 (the yardstick).  What is under test is everything behind `Hip`: which kernel gets which saved tensor, which parent gets
which gradient, which leaf gets which sum.  Each probe ends in the linear loss L = <out, G0> (`linear_loss`), so the upstream
gradient is the test's to choose; two probes keep the real softmax losses.

Instrument 1 (exact): small-integer (or dyadic) operands; the gradients and the forward value must EQUAL float64 autograd.
`prove_probe_exact` asserts on the CPU that every intermediate, every gradient and their absolute-value counterparts are
multiples of 2^-frac_bits below 2^24 (tests/_strict.py: prove_exact).
Instrument 2 (bounded): Gaussian operands; per tensor max|got - g64| <= K * max(E32, 2^-22 max|g64|) with E32 = max|g32 - g64| of the
float32 twin on the CPU.  `margins` reports how close any ReLU-family pre-activation / max-pool window comes to a branch point;
the seeds in SEEDS keep every one further away than 2^-10 max|.|, so no flip allowance is needed.
Every `Twin` takes `defect=` for exactly one wrong closure (DEFECTS): the value of the forward stays, the gradient is the wrong one.

rule -> probes (every name of grad.HOOKED; tests/test_rule_grad_host.py asserts the table is complete):
    as_map                conv_plain, concat_offtape
    as_rows               vit_block
    cast                  vit_block
    flatten               linear_family, tokens_noextra, pool_flatten
    first_row             tokens_cls
    eltwise               conv_plain, se_silu
    add                   fanout
    dropout               dropout_vec, dropout_map, dropout_rows
    drop_path             droppath_seq, droppath_map, droppath_local
    channel_scale         chscale_exact, se_sigmoid, se_hsig, se_silu
    maxpool2d             maxpool
    adaptive_avgpool2d    pool_flatten, chscale_exact, se_sigmoid
    batchnorm             bn_train
    conv2d                conv_plain, conv_variants, conv_bn_act_res, conv_act_res, conv_res_offtape, fanout
    stem_conv_pool        stem
    linear                linear_family, vit_block, tokens_cls
    linear_head           linear_family, vit_block
    layernorm             vit_block
    ln_linear             vit_block
    layernorm_first_row   vit_block
    prep_f32              vit_block, tokens_cls, tokens_noextra
    patch_embed_tokens    vit_block, tokens_cls, tokens_noextra
    qkv_attention         vit_block
    swin_rel_bias         swin_noshift, swin_shift
    swin_window_attention swin_noshift, swin_shift
    patch_merge_gather    patch_merge
    resize_bilinear       resize, loss_pixel
    concat_channels       concat_offtape
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

import eqxvision_amd as eqv
from eqxvision_amd import layers, nn
from eqxvision_amd import random as jr
from eqxvision_amd._module import Module, tree_leaves
from oracle import np_ops as O
from oracle import torch_grad as TG
from tests import _strict as ST

K_BOUND = 8                       # same precision, another summation order (the issue's starting margin; no probe needed more)
FLOOR = 2.0 ** -22
MARGIN = 2.0 ** -10
AUX_WEIGHT = 0.4


def float_leaves(model):
    return [l for l in tree_leaves(model) if isinstance(l, (np.ndarray, eqv._module.DevArray)) and l.dtype.kind == "f"]


# ------------------------------------------------------------------------------------------------ small modules the probes need
class Tokens(Module):
    """The cls token and position embedding of a ViT (models/classification/vit.py: cls_token, pos_embed)."""
    cls_token: Optional[np.ndarray]
    pos_embed: Optional[np.ndarray]

    def __init__(self, D, T, cls=True, pos=True):
        self.cls_token = np.zeros((1, D), np.float32) if cls else None
        self.pos_embed = np.zeros((T, D), np.float32) if pos else None


class RelBias(Module):
    """The relative-position table and index of Swin's window attention (models/classification/swin.py)."""
    relative_position_bias_table: np.ndarray
    relative_position_index: np.ndarray
    window_size: list

    def __init__(self, window, heads):
        from eqxvision_amd.models.classification.swin import _ShiftedWindowAttention
        a = _ShiftedWindowAttention(heads * 4, list(window), [0, 0], heads)
        self.relative_position_bias_table = np.array(a.relative_position_bias_table, np.float32)
        self.relative_position_index = a.relative_position_index
        self.window_size = list(window)

    def get_relative_position_bias(self):
        from eqxvision_amd.models.classification.swin import _get_relative_position_bias
        return _get_relative_position_bias(self.relative_position_bias_table, self.relative_position_index, self.window_size)


class Probe(Module):
    L: dict

    def __init__(self, L, body):
        self.L = L
        self.body = body

    def __call__(self, x, *, key=None):
        return self.body(Hip(), self.L, x, key)


# ------------------------------------------------------------------------------------------------ the library side
class Hip:
    """The composition's entries on the device: the hooked `ops.*` names (looked up at call time) and the library's layers."""

    def __getattr__(self, name):
        from eqxvision_amd import ops
        return getattr(ops, name)

    def fork(self, x):
        return x, x

    def qkv_attention(self, x, lin, heads, scale):
        from eqxvision_amd import ops
        return ops.qkv_attention(x, lin, heads, scale, False)[0]

    def tokens(self, x, tok, conv, n_extra):
        from eqxvision_amd import ops
        cls = ops.prep_f32(tok, "cls_token", None if tok.cls_token is None else tok.cls_token.reshape(-1))
        pos = ops.prep_f32(tok, "pos_embed", tok.pos_embed)
        return ops.patch_embed_tokens(x, conv, cls, pos, n_extra)

    def swin_attention(self, qkv, rel, heads, window, shift):
        from eqxvision_amd import ops
        return ops.swin_window_attention(qkv, ops.swin_rel_bias(rel), heads, window, shift)

    def se(self, x, se):
        return se(x)

    def dropout(self, x, p, key, per_row=False):
        from eqxvision_amd import ops
        if per_row:
            B, N, _ = x.t.shape
            return ops.dropout(x, p, ops.token_keys(key, B, N), per_row=True)
        return nn.Dropout(p)(x, key=key)

    def drop_path(self, x, p, mode, key):
        return layers.DropPath(p, mode=mode)(x, key=key)


def linear_loss(out, G0):
    """L = <out, G0> on a `grad.GTensor`: the value with plain torch on the device, the node hands G0 (times the seed) to out's node.
    `G0` is in the logical layout [B, C, H, W] / [B, N, D] / [B, D]; a map is physically NHWC."""
    from eqxvision_amd import grad
    t = out.act.t
    G = torch.from_numpy(np.ascontiguousarray(G0, np.float32)).to(t.device)
    if out.act.kind == "map":
        G = G.permute(0, 2, 3, 1).contiguous()
    val = (t * G).sum().reshape(1)

    def backward(g):
        s = grad._seed(g)
        return (G if s == 1.0 else G * s,)
    return grad.Scalar(val, grad.Node([out.act.node], backward))


def logical(act) -> np.ndarray:
    t = act.t.detach().cpu().numpy()
    return t.transpose(0, 3, 1, 2) if act.kind == "map" else t


# ------------------------------------------------------------------------------------------------ the torch twin
class TA:
    __slots__ = ("t", "kind", "tape")

    def __init__(self, t, kind, tape=True):
        self.t, self.kind, self.tape = t, kind, tape


def _vg(value, gradpath):
    """`value` in the forward pass, the gradient of `gradpath`: how a defect keeps the forward right and the backward wrong."""
    return gradpath + (value - gradpath).detach()


_ACT = {None: lambda v: v, "none": lambda v: v, "relu": F.relu, "gelu": lambda v: F.gelu(v, approximate="tanh"),
        "hard_swish": F.hardswish, "hard_sigmoid": F.hardsigmoid, "sigmoid": torch.sigmoid, "silu": F.silu}
_BRANCH = {"relu": (0.0,), "hard_swish": (-3.0, 3.0), "hard_sigmoid": (-3.0, 3.0)}

DEFECTS = ("drop_other_key", "drop_no_scale", "drop_phys_order", "droppath_local_as_global", "res_after_act", "res_dropped",
           "fanout_overwrite", "bn_no_stats", "bn_a1_second", "se_no_ds", "cls_one_image", "pos_not_summed", "relidx_not_wrapped",
           "shift_ignored", "concat_offset", "adam_count_minus_1", "aux_seed_1")


class Twin:
    """Every backend entry with plain torch in `dtype`.  `state` carries the BatchNorm running statistics from one call of a model to
    the next; `mag`: parameters replaced by their absolute values and ReLU by the identity (the "mag" counterpart of instrument 1).
    Records every entry's result (`inter`), every ReLU-family pre-activation and max-pool input (`branches`, `pools`)."""

    def __init__(self, model, dtype=torch.float64, defect=None, mag=False, state=None):
        assert defect is None or defect in DEFECTS, defect
        self.dtype, self.defect, self.mag = dtype, defect, mag
        self.leaves = float_leaves(model)
        self.P = {}
        for l in self.leaves:
            a = np.asarray(l, np.float64)
            self.P[id(l)] = torch.from_numpy(np.abs(a) if mag else a).to(dtype).requires_grad_(True)
        self.params = [self.P[id(l)] for l in self.leaves]
        self.state = {} if state is None else state
        self.inter, self.branches, self.pools = [], [], []

    # -- plumbing
    def p(self, leaf):
        return None if leaf is None else self.P[id(leaf)]

    def input(self, x):
        a = np.asarray(x, np.float64)
        return TA(torch.from_numpy(np.abs(a) if self.mag else a).to(self.dtype), "img", tape=False)

    def out(self, t, kind):
        self.inter.append(t)
        return TA(t, kind)

    def act(self, v, act):
        if act in _BRANCH:
            self.branches.append((act, v.detach()))
        if self.mag:
            assert act in (None, "none", "relu"), "exact probes use ReLU only"
            return v
        return _ACT[act](v)

    # -- layout
    def as_map(self, x):
        return TA(x.t, "map", x.tape)

    def as_rows(self, x, keep_fp32=False):
        return x

    def cast(self, x, dtype):
        return x

    def fork(self, x):
        if self.defect == "fanout_overwrite":
            return TA(x.t.detach(), x.kind), x
        return x, x

    def flatten(self, x):
        return self.out(x.t.reshape(x.t.shape[0], -1), "vec")

    def first_row(self, x):
        return self.out(x.t[:, 0], "vec")

    # -- element-wise
    def eltwise(self, x, act):
        return self.out(self.act(x.t, act), x.kind)

    def add(self, a, b, act=None):
        return self.out(self.act(a.t + b.t, act), a.kind)

    def _mask(self, key, keep, x, per_row, phys=False):
        key = np.asarray(key, np.uint32)
        shp = tuple(x.t.shape[1:])
        if per_row:
            B, N, D = x.t.shape
            rows = np.concatenate([O.jax_split(key[b], N) for b in range(B)])
            m = np.stack([O.jax_bernoulli(k, np.float32(keep), (D,)) for k in rows]).reshape(B, N, D)
        elif phys:                               # the stream read in (H, W, C) order instead of the reference's (C, H, W)
            C, H, W = shp
            m = np.stack([O.jax_bernoulli(k, np.float32(keep), (H, W, C)).transpose(2, 0, 1) for k in key])
        else:
            m = np.stack([O.jax_bernoulli(k, np.float32(keep), shp) for k in key])
        return torch.from_numpy(m).to(self.dtype)

    def dropout(self, x, p, key, per_row=False):
        keep = float(np.float32(1.0 - p))
        m = self._mask(key, keep, x, per_row)
        y = x.t * m / keep
        if self.defect == "drop_other_key":
            y = _vg(y, x.t * self._mask(np.asarray(key, np.uint32) ^ np.uint32(1), keep, x, per_row) / keep)
        elif self.defect == "drop_no_scale":
            y = _vg(y, x.t * m)
        elif self.defect == "drop_phys_order" and x.kind == "map":
            y = _vg(y, x.t * self._mask(key, keep, x, per_row, phys=True) / keep)
        return self.out(y, x.kind)

    def drop_path_noise(self, key, keep, mode, C):
        key = np.asarray(key, np.uint32)
        if mode == "global":
            return np.stack([np.full((C,), bool(O.jax_bernoulli(k, np.float32(keep)))) for k in key])
        return np.stack([O.jax_bernoulli(k, np.float32(keep), (C,)) for k in key])

    def drop_path(self, x, p, mode, key):
        keep = float(np.float32(1.0 - p))
        C = x.t.shape[1] if x.kind == "map" else x.t.shape[-1]
        shape = (-1, C, 1, 1) if x.kind == "map" else (-1, 1, C)
        noise = lambda md: torch.from_numpy(self.drop_path_noise(key, keep, md, C)).to(self.dtype).reshape(shape) / keep
        y = x.t * noise(mode)
        if self.defect == "droppath_local_as_global" and mode == "local":
            y = _vg(y, x.t * noise("global"))
        return self.out(y, x.kind)

    def channel_scale(self, x, s):
        st = s.t.reshape(s.t.shape[0], -1, 1, 1)
        if self.defect == "se_no_ds":
            st = st.detach()
        return self.out(x.t * st, "map")

    def se(self, x, se):
        s = self.adaptive_avgpool2d(x, (1, 1))
        s = self.conv2d(s, se.fc1, None, nn.act_name(se.activation.fn))
        s = self.conv2d(s, se.fc2, None, nn.act_name(se.scale_activation.fn))
        return self.channel_scale(x, s)

    # -- pooling, resize, gathers
    def maxpool2d(self, x, kernel_size, stride, padding):
        self.pools.append((x.t.detach(), kernel_size, stride, padding))
        return self.out(F.max_pool2d(x.t, kernel_size, stride, padding), "map")

    def adaptive_avgpool2d(self, x, target, out_fp32=False):
        if tuple(target) == tuple(x.t.shape[2:]):
            return TA(x.t, "map", x.tape)
        return self.out(F.adaptive_avg_pool2d(x.t, target), "map")

    def resize_bilinear(self, x, size, final=False):
        if not final and tuple(size) == tuple(x.t.shape[2:]):
            return TA(x.t, "map", x.tape)
        return self.out(F.interpolate(x.t, size=tuple(size), mode="bilinear", align_corners=False), "img" if final else "map")

    def patch_merge_gather(self, x):
        t = x.t
        return self.out(torch.cat([t[:, :, 0::2, 0::2], t[:, :, 1::2, 0::2], t[:, :, 0::2, 1::2], t[:, :, 1::2, 1::2]], 1), "map")

    def concat_channels(self, xs):
        y = torch.cat([x.t for x in xs], 1)
        if self.defect == "concat_offset":
            y = _vg(y, torch.roll(y, xs[0].t.shape[1], 1))
        return self.out(y, "map")

    # -- normalisation
    def _bn(self, z, bn):
        C = z.shape[1]
        w = self.p(bn.weight) if bn.weight is not None else torch.ones(C, dtype=self.dtype)
        b = self.p(bn.bias) if bn.bias is not None else torch.zeros(C, dtype=self.dtype)
        v = lambda a: a[None, :, None, None]
        if bn.inference:
            rm, rv = (torch.from_numpy(np.asarray(a, np.float64)).to(self.dtype) for a in bn.state_index.value)
            return (z - v(rm)) / torch.sqrt(v(rv) + bn.eps) * v(w) + v(b)
        run = self.state.get(id(bn))
        first = run is None
        sd = {"bn.weight": w, "bn.bias": b}
        if not first:
            sd["bn.running_mean"], sd["bn.running_var"] = run
        new = {}
        y = TG.bn_train(sd, z, "bn", first, bn.momentum, bn.eps, new)
        self.state[id(bn)] = tuple(torch.from_numpy(a).to(self.dtype) for a in new["bn"])
        if self.defect in ("bn_no_stats", "bn_a1_second"):
            mean = z.mean((0, 2, 3))
            var = ((z - v(mean)) ** 2).mean((0, 2, 3))
            rm, rv = self.state[id(bn)]
            if self.defect == "bn_a1_second":         # the gradient of running' = batch, whatever the call
                rm, rv = _vg(rm, mean), _vg(rv, var)
            y = _vg(y, (z - v(rm)) / torch.sqrt(v(rv) + bn.eps) * v(w) + v(b))
        return y

    def batchnorm(self, x, bn, act=None):
        return self.out(self.act(self._bn(x.t, bn), act), x.kind)

    def layernorm(self, x, ln, out_fp32=False):
        return self.out(F.layer_norm(x.t, (x.t.shape[-1],), self.p(ln.weight), self.p(ln.bias), ln.eps), x.kind)

    # -- contractions
    def conv2d(self, x, conv, bn=None, act=None, residual=None):
        b = self.p(conv.bias)
        z = F.conv2d(x.t, self.p(conv.weight), None if b is None else b.reshape(-1), conv.stride, conv.padding, conv.dilation, conv.groups)
        if bn is not None:
            z = self._bn(z, bn)
        if residual is not None:
            r = residual.t
            if self.defect == "res_dropped":
                r = r.detach()
            if self.defect == "res_after_act":        # the residual receives g, not g * act'(.)
                pre = z + r.detach()
                return self.out(self.act(pre, act) + (r - r.detach()), "map")
            z = z + r
        return self.out(self.act(z, act), "map")

    def stem_conv_pool(self, x, conv, bn, act, pool):
        return self.maxpool2d(self.conv2d(x, conv, bn, act), pool.kernel_size, pool.stride, pool.padding)

    def linear(self, x, lin, act=None, residual=None, out_fp32=False):
        t = x.t.permute(0, 2, 3, 1) if x.kind == "map" else x.t
        z = F.linear(t, self.p(lin.weight), self.p(lin.bias))
        if x.kind == "map":
            z = z.permute(0, 3, 1, 2)
        if residual is not None:
            z = z + residual.t
        return self.out(self.act(z, act), x.kind)

    def linear_head(self, x, lin):
        return self.linear(x, lin)

    def ln_linear(self, x, ln, lin, act=None):
        return self.linear(self.layernorm(x, ln), lin, act)

    def layernorm_first_row(self, x, ln, out_fp32=False):
        return self.layernorm(self.first_row(x), ln)

    def tokens(self, x, tok, conv, n_extra):
        y = self.conv2d(x, conv).t.flatten(2).transpose(1, 2)
        B, _, D = y.shape
        if n_extra:
            cls = self.p(tok.cls_token).reshape(1, 1, D)
            rows = [cls if (b == 0 or self.defect != "cls_one_image") else cls.detach() for b in range(B)]
            y = torch.cat([torch.cat(rows, 0), y], 1)
        if tok.pos_embed is not None:
            pos = self.p(tok.pos_embed)[None]
            if self.defect == "pos_not_summed":
                pos = torch.cat([pos] + [pos.detach()] * (B - 1), 0)
            y = y + pos
        return self.out(y, "seq")

    def qkv_attention(self, x, lin, heads, scale):
        B, N, D = x.t.shape
        qkv = self.linear(x, lin).t.reshape(B, N, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
        attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * scale).softmax(-1)
        return self.out((attn @ qkv[2]).transpose(1, 2).reshape(B, N, D), "seq")

    def _window_core(self, t, bias, heads, ws, shift):
        """The shifted-window attention core on NHWC `t` [B, Hf, Wf, 3 C] (tests/_strict.py: swin_bwd64, any dtype)."""
        B, Hf, Wf, C3 = t.shape
        C, (wh, ww) = C3 // 3, ws
        sh = [0 if wh >= Hf else shift[0], 0 if ww >= Wf else shift[1]]
        n, dh, nW = wh * ww, C // heads, (Hf // wh) * (Wf // ww)
        x = torch.roll(t, (-sh[0], -sh[1]), (1, 2)) if sum(sh) > 0 else t
        x = x.reshape(B, Hf // wh, wh, Wf // ww, ww, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, n, 3, heads, dh).permute(2, 0, 3, 1, 4)
        attn = (x[0] * dh ** -0.5) @ x[1].transpose(-2, -1) + bias[None]
        if sum(sh) > 0:
            assert sh[0] > 0 and sh[1] > 0, "the probes shift both axes"
            m = torch.zeros((Hf, Wf), dtype=t.dtype)
            c = 0
            for hh in ((0, -wh), (-wh, -sh[0]), (-sh[0], None)):
                for wl in ((0, -ww), (-ww, -sh[1]), (-sh[1], None)):
                    m[hh[0]:hh[1], wl[0]:wl[1]] = c
                    c += 1
            m = m.reshape(Hf // wh, wh, Wf // ww, ww).permute(0, 2, 1, 3).reshape(nW, n)
            m = m.unsqueeze(1) - m.unsqueeze(2)
            m = m.masked_fill(m != 0, -100.0)
            attn = (attn.reshape(B, nW, heads, n, n) + m[None, :, None]).reshape(-1, heads, n, n)
        y = (attn.softmax(-1) @ x[2]).transpose(1, 2).reshape(B * nW, n, C)
        y = y.reshape(B, Hf // wh, Wf // ww, wh, ww, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hf, Wf, C)
        return torch.roll(y, (sh[0], sh[1]), (1, 2)) if sum(sh) > 0 else y

    def swin_attention(self, qkv, rel, heads, window, shift):
        table = self.p(rel.relative_position_bias_table)
        T, n = table.shape[0], window[0] * window[1]
        raw = torch.from_numpy(np.asarray(rel.relative_position_index).reshape(-1).astype(np.int64))
        gather = lambda idx: table[idx].reshape(n, n, heads).permute(2, 0, 1)
        bias = gather(raw % T)
        if self.defect == "relidx_not_wrapped":
            bias = _vg(bias, gather(raw.clamp(min=0)))
        t = qkv.t.permute(0, 2, 3, 1)
        y = self._window_core(t, bias, heads, window, shift)
        if self.defect == "shift_ignored":
            y = _vg(y, self._window_core(t, bias, heads, window, (0, 0)))
        return self.out(y.permute(0, 3, 1, 2), "map")


# ------------------------------------------------------------------------------------------------ probe bodies
def _conv(cin, cout, k, **kw):
    return nn.Conv2d(cin, cout, k, **kw)


def _bn_inf(C, rng):
    bn = nn.BatchNorm(C, inference=True)
    bn.first_time_index.value = False
    bn.state_index.value = (rng.standard_normal(C).astype(np.float32) * 0.3, rng.uniform(0.5, 1.5, C).astype(np.float32))
    return bn


def b_conv_plain(be, L, x, key):
    y = be.conv2d(be.as_map(x), L["c1"])
    y = be.eltwise(y, "relu")
    return be.conv2d(y, L["c2"])


def b_conv_variants(be, L, x, key):
    y = be.conv2d(x, L["c1"], None, "relu")                 # dilation 2, bias, fused ReLU
    y = be.conv2d(y, L["c2"])                               # groups 4: 2 -> 3 channels per group
    y = be.conv2d(y, L["c3"], None, "relu")                 # depthwise, stride (2, 1)
    return be.conv2d(y, L["c4"])


def b_conv_res(be, L, x, key):
    c0 = be.conv2d(x, L["c0"])
    y = be.conv2d(c0, L["c1"], L.get("bn"), "relu", c0)
    return be.conv2d(y, L["c2"])


def b_conv_res_offtape(be, L, x, key):
    y = be.conv2d(x, L["c1"], None, "relu", x)              # the residual is the raw image: no node, no gradient
    return be.conv2d(y, L["c2"])


def b_fanout(be, L, x, key):
    c0 = be.conv2d(x, L["c0"])
    u, v = be.fork(c0)
    return be.conv2d(be.add(be.conv2d(u, L["ca"]), be.conv2d(v, L["cb"]), "relu"), L["c2"])


def b_bn_train(be, L, x, key):
    y = be.conv2d(x, L["c1"])
    y = be.batchnorm(y, L["bn1"], "silu")                   # affine, fused non-ReLU activation
    y = be.conv2d(y, L["c2"], L["bn2"], "gelu")             # no affine, inside the convolution's rule
    return be.conv2d(y, L["c3"])


def b_linear_family(be, L, x, key):
    y = be.flatten(be.conv2d(x, L["c1"]))                   # HxW map -> (C H W) vector
    h = be.linear(y, L["l1"], "relu")
    h = be.linear(h, L["l2"], None, h)
    return be.linear_head(h, L["l3"])


def b_vit_block(be, L, x, key):
    t = be.as_rows(be.cast(be.tokens(x, L["tok"], L["pe"], 1), "fp32"))
    a = be.qkv_attention(be.layernorm(t, L["ln1"]), L["qkv"], 2, 0.5)
    t = be.linear(a, L["proj"], None, t)
    h = be.ln_linear(t, L["ln2"], L["fc1"], "gelu")
    t = be.linear(h, L["fc2"], None, t)
    return be.linear_head(be.layernorm_first_row(t, L["ln3"]), L["head"])


def b_tokens_cls(be, L, x, key):
    t = be.linear(be.tokens(x, L["tok"], L["pe"], 1), L["l1"], "relu")
    return be.add(be.linear(be.first_row(t), L["l2"]), be.linear(be.flatten(t), L["l3"]))       # the cls row, and every row


def b_tokens_noextra(be, L, x, key):
    return be.linear(be.flatten(be.tokens(x, L["tok"], L["pe"], 0)), L["l1"])


def b_pool_flatten(be, L, x, key):
    y = be.conv2d(x, L["c1"], None, "relu")
    y = be.adaptive_avgpool2d(y, tuple(L["size"]))          # to the input size: the identity
    return be.linear(be.flatten(be.adaptive_avgpool2d(y, (1, 1))), L["l1"])


def b_dropout_vec(be, L, x, key):
    h = be.linear(be.flatten(be.conv2d(x, L["c1"])), L["l1"])
    return be.linear(be.dropout(h, 0.5, jr.split(key, 2)[1]), L["l2"])


def b_dropout_map(be, L, x, key):
    return be.conv2d(be.dropout(be.conv2d(x, L["c1"]), 0.5, jr.split(key, 2)[0]), L["c2"])


def b_dropout_rows(be, L, x, key):
    t = be.linear(be.tokens(x, L["tok"], L["pe"], 0), L["l1"])
    return be.linear(be.dropout(t, 0.5, key, per_row=True), L["l2"])


def b_droppath_seq(be, L, x, key):
    t = be.linear(be.tokens(x, L["tok"], L["pe"], 0), L["l1"])
    return be.linear(be.drop_path(t, 0.5, "global", key), L["l2"])


def b_droppath_map(be, L, x, key):
    return be.conv2d(be.drop_path(be.conv2d(x, L["c1"]), 0.5, L["mode"], key), L["c2"])


def b_chscale(be, L, x, key):
    y = be.conv2d(x, L["c1"], None, "relu")
    s = be.conv2d(be.adaptive_avgpool2d(y, (1, 1)), L["cs"])
    return be.conv2d(be.channel_scale(y, s), L["c2"])


def b_se(be, L, x, key):
    y = be.conv2d(x, L["c1"])
    if L["silu"]:
        y = be.eltwise(y, "silu")
    y = be.se(y, L["se"])
    return be.conv2d(y, L["c2"])


def b_maxpool(be, L, x, key):
    return be.conv2d(be.maxpool2d(be.conv2d(x, L["dw"]), 3, 2, 1), L["c2"])


def b_stem(be, L, x, key):
    return be.conv2d(be.stem_conv_pool(x, L["c1"], L["bn"], "relu", L["pool"]), L["c2"])


def b_swin(be, L, x, key):
    y = be.conv2d(x, L["c1"])
    a = be.swin_attention(be.linear(y, L["qkv"]), L["rel"], 2, (2, 3), tuple(L["shift"]))
    return be.linear(a, L["proj"], None, y)


def b_patch_merge(be, L, x, key):
    return be.linear(be.patch_merge_gather(be.conv2d(x, L["c1"], None, "relu")), L["l1"])


def b_concat(be, L, x, key):
    return be.conv2d(be.concat_channels([be.as_map(x), be.conv2d(x, L["ca"]), be.conv2d(x, L["cb"], None, "relu")]), L["c2"])


def b_resize(be, L, x, key):
    y = be.conv2d(x, L["c1"], None, "relu")
    h, w = L["size"]
    y = be.resize_bilinear(y, (2 * h, 2 * w))
    y = be.resize_bilinear(y, (2 * h, 2 * w))               # the same size: the identity
    return be.resize_bilinear(be.conv2d(y, L["c2"]), (4 * h, 4 * w), final=True)


def b_loss_xent(be, L, x, key):
    y = be.adaptive_avgpool2d(be.conv2d(x, L["c1"], None, "silu"), (1, 1))
    return be.linear_head(be.flatten(y), L["l1"])


def b_loss_pixel(be, L, x, key):
    f = be.conv2d(x, L["c1"], None, "silu")
    size = (2 * L["size"][0], 2 * L["size"][1])
    return (be.resize_bilinear(be.conv2d(f, L["ca"]), size, final=True), be.resize_bilinear(be.conv2d(f, L["co"]), size, final=True))


# ------------------------------------------------------------------------------------------------ the probe table
def _tok_layers(D, hw, patch, cls, pos):
    P = (hw[0] // patch[0]) * (hw[1] // patch[1])
    return {"tok": Tokens(D, P + (1 if cls else 0), cls, pos), "pe": _conv(3, D, patch, stride=patch)}


def _layers(name, rng):
    """The layers of a probe (their values are overwritten by `fill`); B and (H, W) ride along."""
    se = lambda a, g: layers.SqueezeExcitation(8, 4, a, g)
    T = {
        "conv_plain": lambda: (2, (7, 5), {"c1": _conv(3, 8, 3, padding=1), "c2": _conv(8, 6, 3, stride=2, use_bias=False)}),
        "conv_variants": lambda: (2, (5, 6), {"c1": _conv(3, 8, 3, padding=2, dilation=2), "c2": _conv(8, 12, 3, padding=1, groups=4, use_bias=False),
                                               "c3": _conv(12, 12, 3, stride=(2, 1), padding=1, groups=12), "c4": _conv(12, 5, 1)}),
        "conv_bn_act_res": lambda: (2, (6, 5), {"c0": _conv(3, 8, 3, padding=1), "c1": _conv(8, 8, 3, padding=1), "bn": _bn_inf(8, rng),
                                                 "c2": _conv(8, 4, 1)}),
        "conv_act_res": lambda: (2, (6, 5), {"c0": _conv(3, 8, 3, padding=1), "c1": _conv(8, 8, 3, padding=1), "c2": _conv(8, 4, 1)}),
        "conv_res_offtape": lambda: (2, (6, 5), {"c1": _conv(3, 3, 3, padding=1), "c2": _conv(3, 4, 3)}),
        "fanout": lambda: (2, (6, 5), {"c0": _conv(3, 6, 3, padding=1), "ca": _conv(6, 8, 1), "cb": _conv(6, 8, 3, padding=1), "c2": _conv(8, 4, 1)}),
        "bn_train": lambda: (3, (6, 5), {"c1": _conv(3, 8, 3, padding=1), "bn1": nn.BatchNorm(8, "batch"), "c2": _conv(8, 16, 1, use_bias=False),
                                          "bn2": nn.BatchNorm(16, "batch", channelwise_affine=False), "c3": _conv(16, 4, 1)}),
        "linear_family": lambda: (3, (6, 4), {"c1": _conv(3, 4, 3, stride=2), "l1": nn.Linear(8, 10), "l2": nn.Linear(10, 10, use_bias=False),
                                               "l3": nn.Linear(10, 5)}),
        "vit_block": lambda: (2, (6, 4), dict(_tok_layers(8, (6, 4), (2, 2), True, True), ln1=nn.LayerNorm(8), qkv=nn.Linear(8, 24),
                                               proj=nn.Linear(8, 8), ln2=nn.LayerNorm(8), fc1=nn.Linear(8, 16), fc2=nn.Linear(16, 8),
                                               ln3=nn.LayerNorm(8), head=nn.Linear(8, 5))),
        "tokens_cls": lambda: (3, (6, 4), dict(_tok_layers(8, (6, 4), (2, 2), True, True), l1=nn.Linear(8, 8), l2=nn.Linear(8, 5),
                                                l3=nn.Linear(56, 5, use_bias=False))),
        "tokens_noextra": lambda: (2, (6, 4), dict(_tok_layers(4, (6, 4), (2, 2), False, True), l1=nn.Linear(24, 5))),
        "pool_flatten": lambda: (2, (6, 6), {"c1": _conv(3, 8, 3), "size": [4, 4], "l1": nn.Linear(8, 5)}),
        "dropout_vec": lambda: (3, (6, 4), {"c1": _conv(3, 4, 3, stride=2), "l1": nn.Linear(8, 24), "l2": nn.Linear(24, 5)}),
        "dropout_map": lambda: (2, (6, 5), {"c1": _conv(3, 8, 3, padding=1), "c2": _conv(8, 4, 3)}),
        "dropout_rows": lambda: (2, (6, 4), dict(_tok_layers(8, (6, 4), (2, 2), False, False), l1=nn.Linear(8, 12), l2=nn.Linear(12, 5))),
        "droppath_seq": lambda: (3, (6, 4), dict(_tok_layers(8, (6, 4), (2, 2), False, True), l1=nn.Linear(8, 8), l2=nn.Linear(8, 5))),
        "droppath_map": lambda: (3, (6, 5), {"c1": _conv(3, 8, 3, padding=1), "mode": "global", "c2": _conv(8, 4, 3)}),
        "droppath_local": lambda: (3, (6, 5), {"c1": _conv(3, 8, 3, padding=1), "mode": "local", "c2": _conv(8, 4, 3)}),
        "chscale_exact": lambda: (2, (4, 4), {"c1": _conv(3, 8, 3), "cs": _conv(8, 8, 1), "c2": _conv(8, 4, 1)}),
        "se_sigmoid": lambda: (2, (6, 5), {"c1": _conv(3, 8, 3, padding=1), "silu": False, "se": se(nn.relu, nn.sigmoid), "c2": _conv(8, 4, 1)}),
        "se_hsig": lambda: (2, (6, 5), {"c1": _conv(3, 8, 3, padding=1), "silu": False, "se": se(nn.relu, nn.hard_sigmoid), "c2": _conv(8, 4, 1)}),
        "se_silu": lambda: (2, (6, 5), {"c1": _conv(3, 8, 3, padding=1), "silu": True, "se": se(nn.silu, nn.sigmoid), "c2": _conv(8, 4, 1)}),
        "maxpool": lambda: (2, (7, 6), {"dw": _conv(3, 3, 1, groups=3, use_bias=False), "c2": _conv(3, 4, 3, padding=1)}),
        "stem": lambda: (2, (9, 8), {"c1": _conv(3, 8, 3, stride=2, padding=1, use_bias=False), "bn": _bn_inf(8, rng), "pool": nn.MaxPool2d(3, 2, 1),
                                      "c2": _conv(8, 4, 1)}),
        "swin_noshift": lambda: (2, (8, 12), {"c1": _conv(3, 8, 2, stride=2), "qkv": nn.Linear(8, 24), "rel": RelBias((2, 3), 2), "shift": [0, 0],
                                               "proj": nn.Linear(8, 8)}),
        "swin_shift": lambda: (2, (8, 12), {"c1": _conv(3, 8, 2, stride=2), "qkv": nn.Linear(8, 24), "rel": RelBias((2, 3), 2), "shift": [1, 1],
                                             "proj": nn.Linear(8, 8)}),
        "patch_merge": lambda: (2, (6, 4), {"c1": _conv(3, 4, 3, padding=1), "l1": nn.Linear(16, 6)}),
        "concat_offtape": lambda: (2, (6, 5), {"ca": _conv(3, 3, 3, padding=1), "cb": _conv(3, 3, 1), "c2": _conv(9, 4, 3)}),
        "resize": lambda: (2, (5, 4), {"c1": _conv(3, 4, 3), "size": [3, 2], "c2": _conv(4, 3, 1)}),
        "loss_xent": lambda: (3, (6, 5), {"c1": _conv(3, 8, 3), "l1": nn.Linear(8, 5)}),
        "loss_pixel": lambda: (2, (6, 5), {"c1": _conv(3, 8, 3, padding=1), "size": [6, 5], "ca": _conv(8, 5, 1), "co": _conv(8, 5, 1)}),
    }
    return T[name]()


BODY = {"conv_plain": b_conv_plain, "conv_variants": b_conv_variants, "conv_bn_act_res": b_conv_res, "conv_act_res": b_conv_res,
        "conv_res_offtape": b_conv_res_offtape, "fanout": b_fanout, "bn_train": b_bn_train, "linear_family": b_linear_family,
        "vit_block": b_vit_block, "tokens_cls": b_tokens_cls, "tokens_noextra": b_tokens_noextra, "pool_flatten": b_pool_flatten,
        "dropout_vec": b_dropout_vec, "dropout_map": b_dropout_map, "dropout_rows": b_dropout_rows, "droppath_seq": b_droppath_seq,
        "droppath_map": b_droppath_map, "droppath_local": b_droppath_map, "chscale_exact": b_chscale, "se_sigmoid": b_se, "se_hsig": b_se,
        "se_silu": b_se, "maxpool": b_maxpool, "stem": b_stem, "swin_noshift": b_swin, "swin_shift": b_swin, "patch_merge": b_patch_merge,
        "concat_offtape": b_concat, "resize": b_resize, "loss_xent": b_loss_xent, "loss_pixel": b_loss_pixel}
PROBES = tuple(BODY)
# instrument 1: name -> frac_bits (0: integers; 4: an average over 16 pixels; 2: over 4; 8: two bilinear up-samplings at ratio 2)
EXACT = {"conv_plain": 0, "conv_variants": 0, "conv_act_res": 0, "conv_res_offtape": 0, "fanout": 0, "linear_family": 0, "tokens_cls": 0,
         "tokens_noextra": 0, "pool_flatten": 4, "dropout_vec": 0, "dropout_map": 0, "dropout_rows": 0, "droppath_seq": 0, "droppath_map": 0,
         "droppath_local": 0, "chscale_exact": 2, "maxpool": 0, "patch_merge": 0, "concat_offtape": 0, "resize": 8}
BOUNDED = tuple(p for p in PROBES if p != "chscale_exact")
CALLS = {"bn_train": 2}                 # the same model called twice: BatchNorm's a = 1, then a = 1 - momentum
LOSS = {"loss_xent": "xent", "loss_pixel": "pixel"}
# defect -> the probes whose twin must be rejected with it
DEFECT_PROBES = {"drop_other_key": ("dropout_vec", "dropout_map", "dropout_rows"), "drop_no_scale": ("dropout_vec", "dropout_map", "dropout_rows"),
                 "drop_phys_order": ("dropout_map",), "droppath_local_as_global": ("droppath_local",), "res_after_act": ("conv_bn_act_res", "conv_act_res"),
                 "res_dropped": ("conv_bn_act_res", "conv_act_res"), "fanout_overwrite": ("fanout",), "bn_no_stats": ("bn_train",),
                 "bn_a1_second": ("bn_train",), "se_no_ds": ("se_sigmoid", "se_hsig", "se_silu", "chscale_exact"), "cls_one_image": ("tokens_cls", "vit_block"),
                 "pos_not_summed": ("tokens_cls", "tokens_noextra", "vit_block"), "relidx_not_wrapped": ("swin_noshift", "swin_shift"),
                 "shift_ignored": ("swin_shift",), "concat_offset": ("concat_offtape",), "aux_seed_1": ("loss_pixel",)}
# operand seeds per (probe, kind), chosen on the CPU so that the float64 reference keeps the pre-activation margin (bounded) and
# its gradients are non-zero (exact); tests/test_rule_grad_host.py asserts both
SEEDS = {("conv_plain", "gauss"): 6, ("conv_bn_act_res", "gauss"): 2, ("conv_act_res", "gauss"): 11, ("tokens_cls", "gauss"): 1,
         ("maxpool", "gauss"): 6, ("conv_variants", "gauss"): 42, ("stem", "gauss"): 45, ("patch_merge", "gauss"): 2, ("concat_offtape", "gauss"): 1}
KEY_SEED = {}                           # probe -> offset of its PRNG key where the default does not mix kept and dropped samples


def _fill(node, rng, kind):
    """Overwrite every float leaf below `node` in place: integers in {-1, 0, 1} (weights) / [-2, 2] (vectors) for the exact
    instrument, Gaussians scaled by 1 / sqrt(fan-in) for the bounded one; norm weights around 1."""
    if isinstance(node, dict):
        for v in node.values():
            _fill(v, rng, kind)
        return
    if not isinstance(node, Module):
        return
    norm = isinstance(node, (nn.BatchNorm, nn.LayerNorm))
    for f in node.__fields__:
        v = getattr(node, f, None)
        if isinstance(v, (Module, dict)):
            _fill(v, rng, kind)
        elif isinstance(v, np.ndarray) and v.dtype.kind == "f":
            if kind == "int":
                new = rng.integers(-1, 2, v.shape) if v.ndim >= 2 and v.size > 8 else rng.integers(-2, 3, v.shape)
            elif norm:
                new = (1.0 if f == "weight" else 0.0) + 0.3 * rng.standard_normal(v.shape)
            elif v.ndim >= 2 and not isinstance(node, (Tokens, RelBias)):
                new = rng.standard_normal(v.shape) / np.sqrt(max(1, v[0].size))
            else:
                new = 0.5 * rng.standard_normal(v.shape)
            object.__setattr__(node, f, np.ascontiguousarray(new, np.float32))


class Case:
    """One probe with its operands: model, image batches (one per call), keys, cotangent(s) or labels."""

    def __init__(self, name, kind):
        self.name, self.kind = name, kind
        seed = SEEDS.get((name, kind), 0)
        rng = ST.rng_of([sum(map(ord, name)), seed, int(kind == "int")])
        self.B, (H, W), L = _layers(name, rng)
        _fill(L, rng, kind)
        if name == "maxpool" and kind == "int":     # a +-1 per-channel scale of planes of distinct integers: no window holds a tie
            L["dw"].weight = rng.choice(np.array([-1.0, 1.0], np.float32), (3, 1, 1, 1))
        self.model = Probe(L, BODY[name])
        self.calls = CALLS.get(name, 1)
        self.xs = []
        for _ in range(self.calls):
            if kind == "int" and name == "maxpool":
                x = np.stack([rng.permutation(H * W).reshape(H, W) - (H * W) // 2 for _ in range(self.B * 3)]).reshape(self.B, 3, H, W)
            elif kind == "int":
                x = rng.integers(-3, 4, (self.B, 3, H, W))
            else:
                x = rng.standard_normal((self.B, 3, H, W))
            self.xs.append(np.ascontiguousarray(x, np.float32))
        self.keys = jr.split(jr.PRNGKey(KEY_SEED.get(name, 0) + 7), self.B)
        self.loss = LOSS.get(name, "linear")
        self.rng = rng
        self.G0 = None                                # drawn once the output shape is known (the first twin run)
        if self.loss == "xent":
            self.labels = np.arange(self.B) % 5
        if self.loss == "pixel":
            self.labels = rng.integers(0, 5, (self.B, 2 * H, 2 * W))
            self.where = rng.uniform(size=self.labels.shape) > 0.25
            self.labels = np.where(self.where, self.labels, 255)

    def cotangent(self, shape):
        if self.G0 is None:
            g = self.rng.integers(-4, 5, shape) if self.kind == "int" else self.rng.standard_normal(shape)
            self.G0 = np.ascontiguousarray(g, np.float32)
        assert self.G0.shape == tuple(shape)
        return self.G0


def twin_loss(case, tw, out):
    """(forward value tensor, scalar loss) of the twin for this case's loss."""
    if case.loss == "linear":
        G = torch.from_numpy(np.abs(case.cotangent(tuple(out.t.shape))) if tw.mag else case.cotangent(tuple(out.t.shape))).to(tw.dtype)
        return out.t, (out.t * G).sum()
    if case.loss == "xent":
        return out.t, F.cross_entropy(out.t, torch.as_tensor(case.labels, dtype=torch.long), reduction="mean")
    from tests._seg_grad_ref import pixel_losses
    aux, o = out
    la, lo = pixel_losses(aux.t, case.labels, case.where).mean(), pixel_losses(o.t, case.labels, case.where).mean()
    la_s = AUX_WEIGHT * la
    if tw.defect == "aux_seed_1":
        la_s = _vg(la_s, la)
    return torch.cat([aux.t.reshape(-1), o.t.reshape(-1)]), lo + la_s


def run_twin(case, dtype=torch.float64, defect=None, mag=False):
    """[(forward value, loss, [gradient per float leaf], twin)] per call of the model."""
    state, res = {}, []
    for x in case.xs:
        tw = Twin(case.model, dtype, defect, mag, state)
        out = case.model.body(tw, case.model.L, tw.input(x), case.keys)
        val, loss = twin_loss(case, tw, out)
        tw.inter = [t for t in tw.inter if t.requires_grad]
        gi = torch.autograd.grad(loss, tw.params + tw.inter, allow_unused=True)
        n = len(tw.params)
        grads = [np.zeros(tuple(p.shape)) if g is None else g.detach().numpy().astype(np.float64) for p, g in zip(tw.params, gi[:n])]
        tw.inter_grads = [g for g in gi[n:] if g is not None]
        res.append((val.detach().numpy().astype(np.float64), float(loss.detach()), grads, tw))
    return res


def run_hip(case):
    """The same calls on the device -> [(forward value, loss, [gradient per float leaf])]."""
    res = []
    for x in case.xs:
        seen = {}

        @eqv.filter_value_and_grad
        def fn(model, xx):
            out = eqv.vmap(model, axis_name="batch")(xx, key=case.keys)
            if case.loss == "linear":
                seen["val"] = logical(out.act)
                return linear_loss(out, case.cotangent(seen["val"].shape))
            if case.loss == "xent":
                seen["val"] = logical(out.act)
                return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(case.labels, 5)).mean()
            xent = eqv.optim.softmax_cross_entropy_with_integer_labels
            aux, o = out
            seen["val"] = np.concatenate([logical(aux.act).reshape(-1), logical(o.act).reshape(-1)])
            return xent(o, case.labels, axis=1, where=case.where).mean() + AUX_WEIGHT * xent(aux, case.labels, axis=1, where=case.where).mean()

        loss, grads = fn(case.model, x)
        res.append((seen["val"].astype(np.float64), float(loss), [np.asarray(g, np.float64) for g in float_leaves(grads)]))
    return res


# ------------------------------------------------------------------------------------------------ the two instruments
def ratio(got, g64, g32, k=K_BOUND):
    """max|got - g64| / (k max(E32, 2^-22 max|g64|)); inf for a non-finite or mis-shaped `got`."""
    got, g64, g32 = (np.asarray(a, np.float64) for a in (got, g64, g32))
    if got.shape != g64.shape or not np.isfinite(got).all():
        return float("inf")
    e32 = float(np.abs(g32 - g64).max()) if g64.size else 0.0
    bound = k * max(e32, FLOOR * float(np.abs(g64).max()) if g64.size else 0.0)
    err = float(np.abs(got - g64).max()) if g64.size else 0.0
    return err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))


def bounded_ratios(got, r64, r32):
    """Per call: the ratios of the forward value, the loss and every gradient tensor."""
    out = []
    for (v, l, gs), (v64, l64, g64, _), (v32, l32, g32, _) in zip(got, r64, r32):
        assert len(gs) == len(g64)
        out.append([ratio(v, v64, v32), ratio([l], [l64], [l32])] + [ratio(a, b, c) for a, b, c in zip(gs, g64, g32)])
    return out


def exact_mismatches(got, r64):
    """Number of elements that differ, over the forward value and every gradient tensor of every call."""
    bad = 0
    for (v, l, gs), (v64, l64, g64, _) in zip(got, r64):
        for a, b in [(v, v64)] + list(zip(gs, g64)):
            a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
            bad += int(a.size) if a.shape != b.shape else int((a != b).sum())
    return bad


def prove_probe_exact(case):
    """Instrument 1's preconditions on the float64 twin and its absolute-value counterpart."""
    fb = EXACT[case.name]
    ref, mag = run_twin(case), run_twin(case, mag=True)
    for (v, _, gs, tw), (vm, _, gm, twm) in zip(ref, mag):
        hid = [t.detach().numpy() for t in tw.inter + tw.inter_grads + twm.inter + twm.inter_grads]
        ST.prove_exact(f"{case.name}/forward", v, vm, (), hidden=hid, out="fp32", min_nonzero=0.10, frac_bits=fb, hidden_max=ST.ACC_INT_MAX - 1)
        for i, (g, m) in enumerate(zip(gs, gm)):
            assert (np.abs(g) <= m).all(), f"{case.name}: gradient {i} exceeds its absolute-value counterpart"
            ST.prove_exact(f"{case.name}/grad[{i}]", g, m, (), out="fp32", min_nonzero=0.10, frac_bits=fb)
    return ref


def margins(tw):
    """Smallest distance of a ReLU-family pre-activation to a branch point and smallest top-1 / top-2 gap of a max-pool window,
    each relative to max|.| of its tensor (inf when the twin met neither)."""
    worst = float("inf")
    for act, v in tw.branches:
        v = v.double()
        for b in _BRANCH[act]:
            worst = min(worst, float((v - b).abs().min() / v.abs().max()))
    for v, k, s, p in tw.pools:
        v = v.double()
        (kh, kw), (ph, pw) = ST._pair(k), ST._pair(p)
        cols = F.unfold(F.pad(v, (pw, pw, ph, ph), value=-1e30), (kh, kw), stride=s).reshape(v.shape[0], v.shape[1], kh * kw, -1)
        top = cols.topk(2, dim=2).values
        gap = top[:, :, 0] - top[:, :, 1]
        worst = min(worst, float(gap.min() / v.abs().max()))
    return worst


# ------------------------------------------------------------------------------------------------ Adam
def adam_reference(case, steps=3, lr=0.01, dtype=torch.float64, defect=None, written_out=False):
    """`steps` of torch.optim.Adam (or, for the defect, the same update written out) on the twin's parameters, each fed the twin's
    gradients at the parameters it has reached -> the leaves after every step."""
    model = case.model
    leaves = float_leaves(model)
    cur = [np.asarray(l, np.float64) for l in leaves]
    params = [torch.from_numpy(a.copy()).to(dtype).requires_grad_(True) for a in cur]
    opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    mu, nu = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    out = []
    for step in range(1, steps + 1):
        tw = Twin(model, dtype)
        for q, p in zip(tw.params, params):
            q.data.copy_(p.data)
        o = model.body(tw, model.L, tw.input(case.xs[0]), case.keys)
        _, loss = twin_loss(case, tw, o)
        grads = torch.autograd.grad(loss, tw.params)
        if defect is None and not written_out:
            for p, g in zip(params, grads):
                p.grad = g.clone()
            opt.step()
        else:
            assert defect in (None, "adam_count_minus_1")
            c = step if defect is None else step - 1
            with torch.no_grad():
                for p, g, m, v in zip(params, grads, mu, nu):
                    m.mul_(0.9).add_(0.1 * g)
                    v.mul_(0.999).add_(0.001 * g * g)
                    p.sub_(lr * (m / (1 - 0.9 ** c)) / ((v / (1 - 0.999 ** c)).sqrt() + 1e-8))
        out.append([p.detach().numpy().astype(np.float64).copy() for p in params])
    return out
