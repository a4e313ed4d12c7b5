"""Multi-scale deformable attention on the MI355X: the operator, its autograd function and the ``MSDeformAttn`` module.

The reference's only native code is this operator (``downstream/OVIS/mask2former/modeling/pixel_decoder/ops``, CUDA); its Mask2Former /
CTVIS pixel decoder and the ViT-Adapter around the encoder (``models/modeling_timesformer_siglip_adapter.py``; here ``adapter.py``) both run
on it.  Here it
is three HIP entry points (``csrc/sf_msda.hip``): the forward and the backward of the reference op's contract, and a forward with the
front of ``MSDeformAttn.forward`` folded in (softmax over levels x points, sampling locations from reference points and raw offsets,
padding mask), which the module's no-grad path uses.

    from streamformer_amd import MSDeformAttn, ms_deform_attn, as_compiled_op
    sys.modules["MultiScaleDeformableAttention"] = as_compiled_op()      # the reference's own ms_deform_attn_func.py then runs on ROCm

Everything is fp32; tensors are made contiguous; kernels run on torch's current stream.  There is no CPU fallback.
"""
from __future__ import annotations

import math
import types
import weakref
from typing import Any, Sequence, Tuple

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.init import constant_, xavier_uniform_

from . import _native as nat

__all__ = ["ms_deform_attn", "MSDeformAttnFunction", "MSDeformAttn", "as_compiled_op"]

# device tensor -> its values on the host, read back ONCE per tensor object (and in-place version): a repeated or captured call
# with the same shapes tensor does not synchronise
_HOST_INTS: dict = {}


def _host_ints(t: Any) -> Tuple[int, ...]:
    if not isinstance(t, torch.Tensor):
        return tuple(int(v) for row in t for v in (row if isinstance(row, (list, tuple)) else (row,)))
    if t.device.type == "cpu":
        return tuple(int(v) for v in t.reshape(-1).tolist())
    hit = _HOST_INTS.get(id(t))
    if hit is not None and hit[0]() is t and hit[1] == t._version:
        return hit[2]
    vals = tuple(int(v) for v in t.reshape(-1).tolist())
    key = id(t)
    _HOST_INTS[key] = (weakref.ref(t, lambda _, k=key: _HOST_INTS.pop(k, None)), t._version, vals)
    return vals


class _Levels:
    """(H_l, W_l) and level_start_index as the host int arrays the entry points take."""

    def __init__(self, spatial_shapes: Any, level_start_index: Any = None):
        hw = _host_ints(spatial_shapes)
        if len(hw) % 2 or not hw:
            raise ValueError("spatial_shapes must be [n_levels, 2] of (H, W)")
        self.L = len(hw) // 2
        if level_start_index is None:
            start, acc = [], 0
            for l in range(self.L):
                start.append(acc)
                acc += hw[2 * l] * hw[2 * l + 1]
        else:
            start = list(_host_ints(level_start_index))
            if len(start) != self.L:
                raise ValueError(f"level_start_index has {len(start)} entries for {self.L} levels")
        self.hw, self.start = hw, tuple(start)
        self.c_hw, self.c_start = nat.i32_array(hw), nat.i32_array(start)


def _need_gpu(t: torch.Tensor, what: str) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the MI355X: move the tensors with .to('cuda') (there is no CPU fallback)")


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _dims(value, loc, w, lv: _Levels):
    if value.dim() != 4 or loc.dim() != 6 or w.dim() != 5:
        raise ValueError("value [N, S, M, D], sampling_locations [N, Lq, M, L, P, 2], attention_weights [N, Lq, M, L, P]")
    N, S, M, D = value.shape
    _, Lq, _, L, P, two = loc.shape
    if tuple(loc.shape) != (N, Lq, M, L, P, 2) or tuple(w.shape) != (N, Lq, M, L, P) or L != lv.L:
        raise ValueError(f"inconsistent shapes: value {tuple(value.shape)}, sampling_locations {tuple(loc.shape)}, attention_weights "
                         f"{tuple(w.shape)}, {lv.L} levels")
    return N, S, M, D, Lq, L, P


def _forward(value, lv: _Levels, loc, w) -> torch.Tensor:
    _need_gpu(value, "multi-scale deformable attention")
    value, loc, w = _f32(value, "value"), _f32(loc, "sampling_locations"), _f32(w, "attention_weights")
    N, S, M, D, Lq, L, P = _dims(value, loc, w, lv)
    out = torch.empty(N, Lq, M * D, device=value.device, dtype=torch.float32)
    nat.launch(value.device, nat.lib.sf_op_msda_forward, value.data_ptr(), lv.c_hw, lv.c_start, loc.data_ptr(), w.data_ptr(), out.data_ptr(),
               N, S, M, D, Lq, L, P)
    return out


def _backward(value, lv: _Levels, loc, w, grad_out):
    _need_gpu(value, "multi-scale deformable attention")
    value, loc, w, grad_out = _f32(value, "value"), _f32(loc, "sampling_locations"), _f32(w, "attention_weights"), _f32(grad_out, "grad_output")
    N, S, M, D, Lq, L, P = _dims(value, loc, w, lv)
    if tuple(grad_out.shape) != (N, Lq, M * D):
        raise ValueError(f"grad_output {tuple(grad_out.shape)} is not [N, Lq, M * D] = {(N, Lq, M * D)}")
    gv, gl, gw = torch.empty_like(value), torch.empty_like(loc), torch.empty_like(w)
    nat.launch(value.device, nat.lib.sf_op_msda_backward, value.data_ptr(), lv.c_hw, lv.c_start, loc.data_ptr(), w.data_ptr(), grad_out.data_ptr(),
               gv.data_ptr(), gl.data_ptr(), gw.data_ptr(), N, S, M, D, Lq, L, P)
    return gv, gl, gw


class MSDeformAttnFunction(Function):
    """The reference's ``MSDeformAttnFunction`` (functions/ms_deform_attn_func.py:32-49) on the HIP kernels.  ``im2col_step`` is accepted
    and ignored: the kernels take the whole batch in one launch."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, im2col_step=None):
        ctx.levels = _Levels(value_spatial_shapes, value_level_start_index)
        out = _forward(value, ctx.levels, sampling_locations, attention_weights)
        ctx.save_for_backward(value, sampling_locations, attention_weights)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, loc, w = ctx.saved_tensors
        gv, gl, gw = _backward(value, ctx.levels, loc, w, grad_output)
        return gv, None, None, gl, gw, None


def ms_deform_attn(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step=None):
    """out [N, Lq, M * D] of value [N, S, M, D] sampled at sampling_locations [N, Lq, M, L, P, 2] with attention_weights
    [N, Lq, M, L, P]; differentiable in all three.  ``spatial_shapes`` ([L, 2] of (H, W)) and ``level_start_index`` ([L], or None: the
    running sum) may be Python lists, CPU tensors or device tensors; a device tensor is read back once and remembered by identity."""
    return MSDeformAttnFunction.apply(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step)


def as_compiled_op():
    """A stand-in for the reference's compiled extension ``MultiScaleDeformableAttention`` (src/vision.cpp): the two functions its
    ``ms_deform_attn_func.py`` calls, with the same arguments and results."""
    mod = types.ModuleType("MultiScaleDeformableAttention")

    def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step=None):
        return _forward(value, _Levels(spatial_shapes, level_start_index), sampling_loc, attn_weight)

    def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step=None):
        return _backward(value, _Levels(spatial_shapes, level_start_index), sampling_loc, attn_weight, grad_output)

    mod.ms_deform_attn_forward = ms_deform_attn_forward
    mod.ms_deform_attn_backward = ms_deform_attn_backward
    return mod


class MSDeformAttn(nn.Module):
    """The reference's ``MSDeformAttn`` (modules/ms_deform_attn.py:34-125): same parameter tree, state-dict keys, initialisation and
    ``forward`` signature.

    ``ratio`` is accepted and ignored, exactly as the reference's live class does (its ViT-Adapter passes ``deform_ratio=0.5``, which
    only the commented-out variant of the class would honour): value and output projections stay d_model wide.

    Two paths.  Without gradients the four projections run on the library's GEMMs in ``compute_dtype`` ("fp32", the default: bf16x3
    operands, fp32-accurate; "bf16": one pass of bf16 operands) — sampling offsets and attention logits as ONE GEMM over the
    concatenated weights — followed by the fused kernel, which does the softmax, the sampling locations and the padding mask itself.
    With gradients the projections and the softmax are plain torch and the sampling is ``MSDeformAttnFunction``; a native backward of the
    projections is not part of this module.  The no-grad path needs d_model to be a multiple of 64 (the GEMM kernels' k-step).
    """

    def __init__(self, d_model: int = 256, n_levels: int = 4, n_heads: int = 8, n_points: int = 4, ratio: float = 1.0,
                 compute_dtype: Any = "fp32"):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError("d_model must be divisible by n_heads, but got {} and {}".format(d_model, n_heads))
        self._compute = nat.compute_mode(compute_dtype)
        self.im2col_step = 128
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.compute_dtype = compute_dtype
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)
        self._native = nat.PackedHandle(noun="MSDeformAttn")       # no handle of its own: the GEMMs' workspace
        self._front, self._front_token = None, None
        self._reset_parameters()

    def _reset_parameters(self) -> None:
        constant_(self.sampling_offsets.weight.data, 0.)
        thetas = torch.arange(self.n_heads, dtype=torch.float32) * (2.0 * math.pi / self.n_heads)
        grid_init = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid_init = (grid_init / grid_init.abs().max(-1, keepdim=True)[0]).view(self.n_heads, 1, 1, 2).repeat(1, self.n_levels, self.n_points, 1)
        for i in range(self.n_points):
            grid_init[:, :, i, :] *= i + 1
        with torch.no_grad():
            self.sampling_offsets.bias = nn.Parameter(grid_init.view(-1))
        constant_(self.attention_weights.weight.data, 0.)
        constant_(self.attention_weights.bias.data, 0.)
        xavier_uniform_(self.value_proj.weight.data)
        constant_(self.value_proj.bias.data, 0.)
        xavier_uniform_(self.output_proj.weight.data)
        constant_(self.output_proj.bias.data, 0.)

    # ---- no-grad path ------------------------------------------------------------------------------
    def _linear(self, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, resid: torch.Tensor = None) -> torch.Tensor:
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, device=x.device, dtype=torch.float32)
        nbytes = nat.lib.sf_op_linear_workspace_bytes(M, N, K)
        ws = self._native.workspace(nbytes, x.device)
        nat.launch(x.device, nat.lib.sf_op_linear, x.data_ptr(), w.data_ptr(), b.data_ptr(), nat.ptr(resid), 1.0, 0, y.data_ptr(), M, N, K, self._compute,
                   workspace=ws)
        return y

    def _front_weights(self, dev) -> Tuple[torch.Tensor, torch.Tensor]:
        """[sampling_offsets; attention_weights] as one [3 * M * L * P, d_model] weight and bias, rebuilt when a parameter changes."""
        ps = [self.sampling_offsets.weight, self.sampling_offsets.bias, self.attention_weights.weight, self.attention_weights.bias]
        token = nat.weights_token(dev, ps)
        if token != self._front_token:
            with torch.no_grad():
                self._front = (torch.cat([ps[0], ps[2]]).float().contiguous(), torch.cat([ps[1], ps[3]]).float().contiguous())
            self._front_token = token
        return self._front

    def __getstate__(self):
        return dict(self.__dict__, _front=None, _front_token=None)      # a copy concatenates its own

    def _forward_native(self, query, reference_points, input_flatten, lv: _Levels, input_padding_mask, resid=None):
        """``resid`` [N, Lq, d_model] fp32 contiguous (the ViT-Adapter's extractors): added to the result by the output GEMM's epilogue."""
        N, Lq, Cq = query.shape
        S = input_flatten.shape[1]
        Mh, L, P, D = self.n_heads, self.n_levels, self.n_points, self.d_model // self.n_heads
        if self.d_model % 64:
            raise ValueError(f"the no-grad path of MSDeformAttn needs d_model % 64 == 0 (the GEMM kernels' k-step), got {self.d_model}")
        dev = query.device
        with torch.cuda.device(dev):
            value = self._linear(_f32(input_flatten, "input_flatten").reshape(N * S, Cq), self.value_proj.weight.detach(), self.value_proj.bias.detach())
            fw, fb = self._front_weights(dev)
            front = self._linear(_f32(query, "query").reshape(N * Lq, Cq), fw, fb)           # [N * Lq, 3 * M * L * P]: offsets, then logits
            n_off = Mh * L * P * 2
            ref = _f32(reference_points, "reference_points")
            pad = None
            if input_padding_mask is not None:
                pad = input_padding_mask.to(torch.uint8).contiguous()
                if tuple(pad.shape) != (N, S):
                    raise ValueError(f"input_padding_mask {tuple(pad.shape)} is not [N, S] = {(N, S)}")
            ctx = torch.empty(N * Lq, self.d_model, device=dev, dtype=torch.float32)
            nat.launch(dev, nat.lib.sf_op_msda_forward_fused, value.data_ptr(), nat.ptr(pad), lv.c_hw, lv.c_start, front.data_ptr(), front.shape[1],
                       front.data_ptr() + 4 * n_off, front.shape[1], ref.data_ptr(), ref.shape[-1], ctx.data_ptr(), N, S, Mh, D, Lq, L, P)
            return self._linear(ctx, self.output_proj.weight.detach(), self.output_proj.bias.detach(), resid).view(N, Lq, self.d_model)

    # ---- grad path ---------------------------------------------------------------------------------
    def _forward_autograd(self, query, reference_points, input_flatten, lv: _Levels, input_padding_mask):
        N, Lq, _ = query.shape
        S = input_flatten.shape[1]
        Mh, L, P = self.n_heads, self.n_levels, self.n_points
        value = self.value_proj(input_flatten)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], float(0))
        value = value.view(N, S, Mh, self.d_model // Mh)
        offsets = self.sampling_offsets(query).view(N, Lq, Mh, L, P, 2)
        weights = torch.softmax(self.attention_weights(query).view(N, Lq, Mh, L * P), -1).view(N, Lq, Mh, L, P)
        if reference_points.shape[-1] == 2:
            normalizer = torch.tensor([[lv.hw[2 * l + 1], lv.hw[2 * l]] for l in range(L)], dtype=query.dtype, device=query.device)
            locations = reference_points[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
        else:
            locations = reference_points[:, :, None, :, None, :2] + offsets / P * reference_points[:, :, None, :, None, 2:] * 0.5
        out = MSDeformAttnFunction.apply(value, lv.hw, lv.start, locations, weights, self.im2col_step)
        return self.output_proj(out)

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index, input_padding_mask=None):
        """query [N, Lq, C]; reference_points [N, Lq, n_levels, 2] in [0, 1] or [N, Lq, n_levels, 4] boxes; input_flatten [N, S, C];
        input_spatial_shapes [n_levels, 2] of (H, W); input_level_start_index [n_levels]; input_padding_mask [N, S], True = padding.
        Returns [N, Lq, C]."""
        if query.device.type != "cuda":
            raise RuntimeError("MSDeformAttn runs on the MI355X: move the module and its inputs with .to('cuda') (there is no CPU fallback)")
        lv = _Levels(input_spatial_shapes, input_level_start_index)
        N, Lq, _ = query.shape
        S = input_flatten.shape[1]
        if lv.L != self.n_levels or sum(lv.hw[2 * l] * lv.hw[2 * l + 1] for l in range(lv.L)) != S:
            raise ValueError(f"input_spatial_shapes {lv.hw} do not describe {self.n_levels} levels of {S} pixels in all")
        if reference_points.shape[-1] not in (2, 4):
            raise ValueError("Last dim of reference_points must be 2 or 4, but get {} instead.".format(reference_points.shape[-1]))
        tensors: Sequence[torch.Tensor] = (query, reference_points, input_flatten, *self.parameters())
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            return self._forward_autograd(query, reference_points, input_flatten, lv, input_padding_mask)
        return self._forward_native(query, reference_points, input_flatten, lv, input_padding_mask)
