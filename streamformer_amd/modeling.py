"""Python mirror of the reference encoder module, backed by the HIP library.

Drop-in surface (reference ``models/modeling_timesformer_siglip.py``):

* ``TimesformerMultiTaskingModelSigLIP`` IS a ``torch.nn.Module`` whose parameter tree has the reference's names
  (``embeddings.position_embeddings`` ... ``head.mlp.fc2.bias``, the unused ``...attention.mask`` buffers included), so a
  wrapper can hold it as ``self.timesformer = TimesformerMultiTaskingModelSigLIP(config)`` (``:1362``), ``.to(device)``
  it, ``state_dict()`` / ``load_state_dict()`` it with or without the ``timesformer.`` prefix, and read
  ``next(model.parameters()).device / .dtype`` (``vqa_enc:1574-1581``).  The ``nn.Parameter`` tensors are the fp32
  (or bf16 / fp16 after ``.to(dtype)``) master copy; the library packs its own bf16 operands from them whenever they
  change (tracked through the tensors' version counters).
* ``TimesformerMultiTaskingModelSigLIP.from_pretrained(dir)``           (``:1066-1075``, HF classmethod)
* ``model(pixel_values[B,T,3,H,W], output_attentions=None, output_hidden_states=None,
  return_dict=None)`` -> object with ``last_hidden_state (B,T,N,D)``, ``pooler_output (B,T,D)``,
  ``hidden_states`` (L+1 x ``(B, N*T, D)`` patch-major, ``:1352``), ``attentions``; a tuple when
  ``return_dict=False`` (``:1299-1354``)
* streaming kwargs of the VideoQA copy: ``past_key_values``, ``use_cache``, ``cache_position``, also together with
  ``output_hidden_states=True`` (the tower's call form, ``downstream/VideoQA/.../timesformer_encoder.py:1316-1392, 1536``)
* sub-modules with the reference's call shapes: ``model.embeddings(pixel_values)``, ``model.encoder(h, num_frames=T)``,
  ``model.encoder.layer[i](h, T, output_attentions=False)``, ``model.post_layernorm(x)``, ``model.head(x)``
* ``add_lora_spatial()``, ``frozen_spatial()`` (``:1271-1297``), ``.config``, ``.device``, ``.dtype``.

All arithmetic of the forward runs in ``libstreamformer_hip.so`` through ``_native`` (ctypes);
torch supplies device memory, streams and the tensor container only.  There is no CPU or eager
fallback: without the library or without a GPU the forward raises.
"""
from __future__ import annotations

import os
import weakref
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import _native as nat
from .configuration import LORA_RANK, StreamformerConfig

_ACT_CODES = {"gelu": 0, "gelu_new": 1, "gelu_pytorch_tanh": 1, "relu": 2}
_TORCH2SF = {torch.uint8: nat.SF_U8, torch.float32: nat.SF_F32, torch.bfloat16: nat.SF_BF16, torch.float16: nat.SF_F16,
             torch.float64: nat.SF_F64}


class ModelOutput(OrderedDict):
    """Attribute + key + index access, like ``transformers.utils.ModelOutput`` (None fields are skipped
    by integer indexing / ``to_tuple``)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __getitem__(self, k):
        if isinstance(k, (int, slice)):
            return self.to_tuple()[k]
        return super().__getitem__(k)

    def to_tuple(self) -> tuple:
        return tuple(v for v in self.values() if v is not None)


def BaseModelOutputWithPooling(last_hidden_state, pooler_output, hidden_states=None, attentions=None):
    return ModelOutput(last_hidden_state=last_hidden_state, pooler_output=pooler_output,
                       hidden_states=hidden_states, attentions=attentions)


def BaseModelOutputWithPast(last_hidden_state, past_key_values=None, hidden_states=None, attentions=None,
                            pooler_output=None):
    # vqa_enc:1387-1392 drops pooler_output; it is kept here as an extra trailing field.
    return ModelOutput(last_hidden_state=last_hidden_state, past_key_values=past_key_values,
                       hidden_states=hidden_states, attentions=attentions, pooler_output=pooler_output)


def _stale_message(what: str, remedy: str) -> str:
    return (f"this {what} belongs to weights / a compute mode / a device the model has since left (load_state_dict, "
            f"set_compute_dtype or .to() re-packed it): {remedy}")


_SNAPSHOT_FIELDS = tuple(n for n, _ in nat.SfCacheStreamMeta._fields_)


class StreamSnapshot:
    """One parked stream of a ``StreamCache``: the K/V rows of the frames it holds (``blob``, a flat uint8 tensor on the GPU or the
    host) and ``meta``, the plain-int mirror of ``sf_cache_stream_meta`` that says what the blob is and where it may go back.

    Plain data: it pickles (``torch.save(snapshot)``), and ``state_dict()`` / ``from_state_dict()`` give the form that
    ``torch.load(..., weights_only=True)`` accepts.  ``StreamCache.restore()`` takes it back, in this process or another."""

    def __init__(self, blob: torch.Tensor, meta: Dict[str, int], _origin=None):
        self.blob, self.meta = blob, dict(meta)
        self._origin = _origin      # (weakref of the model, its pack epoch) while in the process that took it; never pickled
        self._validate()

    def _validate(self) -> None:
        m, b = self.meta, self.blob
        missing = [k for k in _SNAPSHOT_FIELDS if k not in m]
        if missing or len(m) != len(_SNAPSHOT_FIELDS):
            raise ValueError(f"snapshot meta must hold exactly {_SNAPSHOT_FIELDS}; missing {missing}, "
                             f"unknown {sorted(set(m) - set(_SNAPSHOT_FIELDS))}")
        for k in _SNAPSHOT_FIELDS:
            if not isinstance(m[k], int) or isinstance(m[k], bool) or m[k] < 0:
                raise ValueError(f"snapshot meta field {k!r} must be a non-negative int, got {m[k]!r}")
        if m["format"] != nat.SF_STREAM_BLOB_KV1:
            raise ValueError(f"snapshot meta field 'format' is 0x{m['format']:08x}, not the blob format this version reads "
                             f"(0x{nat.SF_STREAM_BLOB_KV1:08x})")
        if m["elem_bytes"] != (4 if m["compute"] == nat.SF_COMPUTE_BF16X3 else 2) or m["compute"] not in (0, 1):
            raise ValueError(f"snapshot meta fields 'compute' = {m['compute']} and 'elem_bytes' = {m['elem_bytes']} disagree")
        if m["max_frames"] < 1 or m["frames_held"] != min(m["frames_seen"], m["max_frames"]):
            raise ValueError(f"snapshot meta field 'frames_held' = {m['frames_held']} is not min(frames_seen = {m['frames_seen']}, "
                             f"max_frames = {m['max_frames']})")
        want = m["layers"] * m["frames_held"] * m["patches"] * 2 * m["hidden_size"] * m["elem_bytes"]
        if m["blob_bytes"] != want:
            raise ValueError(f"snapshot meta field 'blob_bytes' = {m['blob_bytes']}, but its geometry makes {want}")
        if not isinstance(b, torch.Tensor) or b.dtype != torch.uint8 or b.dim() != 1 or not b.is_contiguous():
            raise ValueError("snapshot blob must be a contiguous 1-D uint8 tensor")
        if b.numel() != want:
            raise ValueError(f"snapshot blob holds {b.numel()} bytes, its meta describes {want} (truncated?)")

    @property
    def nbytes(self) -> int:
        return self.blob.numel()

    @property
    def frames_seen(self) -> int:
        return self.meta["frames_seen"]

    @property
    def device(self) -> torch.device:
        return self.blob.device

    def to(self, device) -> "StreamSnapshot":
        """The same snapshot with its blob on ``device``; a blob that leaves the GPU lands in pinned host memory."""
        device = torch.device(device)
        if device.type == self.blob.device.type and (device.index is None or device.index == self.blob.device.index):
            return self
        if device.type == "cpu" and self.blob.is_cuda:
            blob = torch.empty(self.blob.numel(), dtype=torch.uint8, pin_memory=True)
            blob.copy_(self.blob)
        else:
            blob = self.blob.to(device)
        return StreamSnapshot(blob, self.meta, self._origin)

    def state_dict(self) -> Dict[str, Any]:
        return {"blob": self.blob, "meta": dict(self.meta)}

    @classmethod
    def from_state_dict(cls, sd: Dict[str, Any]) -> "StreamSnapshot":
        return cls(sd["blob"], sd["meta"])

    def __getstate__(self):
        return self.state_dict()

    def __setstate__(self, d):
        self.blob, self.meta, self._origin = d["blob"], dict(d["meta"]), None
        self._validate()

    def __repr__(self) -> str:
        m = self.meta
        return (f"StreamSnapshot(frames_seen={m['frames_seen']}, frames_held={m['frames_held']}, max_frames={m['max_frames']}, "
                f"nbytes={self.nbytes}, device={self.blob.device})")


class StreamCache:
    """Temporal KV-cache of ``batch`` streams: the ``past_key_values`` object of the streaming forward.

    Library-owned device memory (``sf_cache``); mirrors the two things the reference uses of HF's
    ``DynamicCache``: ``get_seq_length()`` (vqa_enc:328-331) and being threaded through calls.
    A cache belongs to the packed weights it was created against: when the model re-packs (new weights, another
    compute mode, another device) the cache is invalidated and the next use raises instead of reading freed memory.

    Every stream (slab) of a batched cache keeps its own position.  The plain call advances all of them together and needs them
    level; ``forward(..., stream_ids=[...])`` advances any subset, each from where it stands.  ``acquire()`` / ``release()`` hand
    slabs out to sessions that come and go."""

    def __init__(self, model: "TimesformerMultiTaskingModelSigLIP", batch: int, max_frames: int, H: int, W: int,
                 policy: str = "stop"):
        if policy not in ("stop", "slide"):
            raise ValueError("policy must be 'stop' (raise at capacity, like the reference) or 'slide' (sliding window over the last max_frames frames)")
        self._model = weakref.ref(model)
        self._h = nat.OwnedHandle(nat.lib.sf_cache_destroy, "StreamCache")
        nat.check(nat.lib.sf_cache_create(model._handle, batch, max_frames, H, W, nat.C.byref(self._h)))
        self.batch, self.max_frames, self.H, self.W, self.policy = batch, max_frames, H, W, policy
        self._free = list(range(batch))      # slabs no session holds, lowest first (acquire / release)
        if policy == "slide":
            nat.check(nat.lib.sf_cache_set_policy(self._h, 1))
        model._native.dependents.add(self._h)      # invalidated (released) with the packing it was created against

    @property
    def valid(self) -> bool:
        return bool(self._h)

    def _require(self):
        if not self._h:
            raise RuntimeError(_stale_message("past_key_values", "start a new cache"))
        return self._h

    def get_seq_length(self, layer_idx: int = 0, stream: Optional[int] = None) -> int:
        """Frames the cache holds (HF ``DynamicCache`` semantics): never more than ``max_frames`` under the sliding window.
        ``stream``: of that stream; otherwise of the longest one."""
        seen = self.frames_seen if stream is None else self.frames_seen_per_stream[self._check_stream(stream)]
        return min(seen, self.max_frames)

    @property
    def frames_seen(self) -> int:
        """Frames streamed through this cache since its creation / last ``reset()`` (the longest stream's count)."""
        return nat.lib.sf_cache_length(self._require())

    @property
    def frames_seen_per_stream(self) -> List[int]:
        h = self._require()
        return [nat.lib.sf_cache_stream_length(h, i) for i in range(self.batch)]

    def _check_stream(self, stream: int) -> int:
        if not isinstance(stream, int) or isinstance(stream, bool) or not 0 <= stream < self.batch:
            raise ValueError(f"stream must be an int in 0..{self.batch - 1} (this cache holds {self.batch} streams), got {stream!r}")
        return stream

    def reset(self, stream: Optional[int] = None) -> None:
        """Forget every stream's frames, or those of ``stream`` alone (the others keep their positions)."""
        if stream is None:
            nat.check(nat.lib.sf_cache_reset(self._require()))
        else:
            nat.check(nat.lib.sf_cache_reset_stream(self._require(), self._check_stream(stream)))

    def acquire(self) -> int:
        """A free slab for a new session (the lowest free index).  Raises when every slab is held."""
        return _slab_acquire(self._free, self.batch)

    def release(self, stream: int) -> None:
        """Return a slab: it is reset and may be handed out again."""
        _slab_release(self._free, self._check_stream(stream))
        self.reset(stream)

    @property
    def nbytes(self) -> int:
        return nat.lib.sf_cache_bytes(self._require())

    def snapshot(self, stream: int, device: Any = None) -> StreamSnapshot:
        """Park ``stream``: its cached K/V (the frames it holds, all layers) packed into one blob by one kernel launch.  The stream
        itself stays as it is — ``release()`` it to hand the slab on.  ``device="cpu"``: the blob is then moved to pinned host
        memory; by default it stays on the GPU."""
        h = self._require()
        model = self._model()
        stream = self._check_stream(stream)
        nbytes = nat.sized(nat.lib.sf_cache_stream_blob_bytes, h, stream)
        meta = nat.SfCacheStreamMeta()
        dev = model.device
        with torch.cuda.device(dev):
            blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)        # the snapshot keeps it: exactly the blob, no floor
            nat.launch(dev, nat.lib.sf_cache_export_stream, model._handle, h, stream, blob.data_ptr(), nbytes, nat.C.byref(meta))
        snap = StreamSnapshot(blob, {k: int(getattr(meta, k)) for k in _SNAPSHOT_FIELDS}, (weakref.ref(model), model._pack_epoch))
        return snap if device is None else snap.to(device)

    def restore(self, snapshot: StreamSnapshot, stream: Optional[int] = None) -> int:
        """Resume a parked stream in slab ``stream`` of this cache (a slab the caller holds), or in a slab ``acquire()``d here when
        ``stream`` is None; returns the slab index.  Every frame goes back to the ring slot it came from and the frame count is
        restored, so the continuation — the ordinary ``forward(..., past_key_values=cache, stream_ids=[...])`` — is bit-identical
        to the uninterrupted stream.  Any slab of any cache of the same weights, compute mode, resolution, ``max_frames`` and
        policy will do (any ``batch_size``); restoring one snapshot into two slabs forks the stream.  A refusal leaves the slab
        as it was, and an auto-acquired slab goes back to the free list."""
        if not isinstance(snapshot, StreamSnapshot):
            raise TypeError("restore() takes the StreamSnapshot that StreamCache.snapshot() returned")
        model = self._model()
        if model is not None and self._h:
            model._sync()               # a pending re-pack happens now: it invalidates this cache and ages the model's snapshots
        h = self._require()
        snapshot._validate()
        origin = snapshot._origin
        if origin is not None and origin[0]() is model and origin[1] != model._pack_epoch:
            raise RuntimeError(_stale_message("snapshot", "stream its frames again"))
        own = stream is None
        sid = self.acquire() if own else self._check_stream(stream)
        try:
            dev = model.device
            with torch.cuda.device(dev):
                blob = snapshot.blob.to(dev, non_blocking=True)
                meta = nat.SfCacheStreamMeta(**snapshot.meta)
                nat.launch(dev, nat.lib.sf_cache_import_stream, model._handle, h, sid, blob.data_ptr(), blob.numel(), nat.C.byref(meta))
        except Exception:
            if own:
                _slab_release(self._free, sid)
            raise
        return sid


def _slab_acquire(free: List[int], batch: int) -> int:
    if not free:
        raise RuntimeError(f"all {batch} streams of this cache are in use: release() one, or create the cache with a larger "
                           "batch_size")
    return free.pop(0)


def _slab_release(free: List[int], stream: int) -> None:
    if stream in free:
        raise ValueError(f"stream {stream} is not acquired (released twice?)")
    free.append(stream)
    free.sort()


def expected_keys(cfg: StreamformerConfig, lora: Optional[bool] = None) -> "OrderedDict[str, Tuple[int, ...]]":
    """Parameter names and shapes of the reference module."""
    lora = bool(cfg.add_lora_spatial) if lora is None else lora
    D, I, P, C, N, T = (cfg.hidden_size, cfg.intermediate_size, cfg.patch_size, cfg.num_channels,
                        cfg.num_patches, cfg.num_frames)
    k: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    k["embeddings.position_embeddings"] = (1, N, D)
    k["embeddings.time_embeddings"] = (1, T, D)
    k["embeddings.patch_embeddings.projection.weight"] = (D, C, P, P)
    k["embeddings.patch_embeddings.projection.bias"] = (D,)

    def lin(p, o, i, bias=True):
        k[p + ".weight"] = (o, i)
        if bias:
            k[p + ".bias"] = (o,)

    def ln(p):
        k[p + ".weight"] = (D,)
        k[p + ".bias"] = (D,)

    # order = the reference's named_parameters() (tests/golden/f12_param_order.json, pinned by oracle/make_golden_param_order.py):
    # torch.optim state ids, DDP buckets and checkpoint-*.pth optimizer entries follow it
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layer.{i}."
        k[p + "temporal_attention_gating"] = ()
        lin(p + "attention.attention.qkv", 3 * D, D, cfg.qkv_bias)
        if lora:
            k[p + "attention.attention.qkv_lora_a.weight"] = (LORA_RANK, D)
            k[p + "attention.attention.qkv_lora_b.weight"] = (3 * D, LORA_RANK)
        lin(p + "attention.output.dense", D, D)
        if lora:
            k[p + "attention.output.dense_lora_a.weight"] = (LORA_RANK, D)
            k[p + "attention.output.dense_lora_b.weight"] = (D, LORA_RANK)
        lin(p + "intermediate.dense", I, D)
        lin(p + "output.dense", D, I)
        ln(p + "layernorm_before")
        ln(p + "layernorm_after")
        ln(p + "temporal_layernorm")
        lin(p + "temporal_attention.attention.qkv", 3 * D, D, cfg.qkv_bias)
        lin(p + "temporal_attention.output.dense", D, D)
        lin(p + "temporal_dense", D, D)
    ln("post_layernorm")
    k["head.probe"] = (1, 1, D)
    k["head.attention.in_proj_weight"] = (3 * D, D)
    k["head.attention.in_proj_bias"] = (3 * D,)
    lin("head.attention.out_proj", D, D)
    ln("head.layernorm")
    lin("head.mlp.fc1", I, D)
    lin("head.mlp.fc2", D, I)
    return k


def _lora_keys(cfg: StreamformerConfig, i: int) -> "OrderedDict[str, Tuple[int, ...]]":
    D, p = cfg.hidden_size, f"encoder.layer.{i}."
    return OrderedDict([(p + "attention.attention.qkv_lora_a.weight", (LORA_RANK, D)),
                        (p + "attention.attention.qkv_lora_b.weight", (3 * D, LORA_RANK)),
                        (p + "attention.output.dense_lora_a.weight", (LORA_RANK, D)),
                        (p + "attention.output.dense_lora_b.weight", (D, LORA_RANK))])


def normalize_checkpoint_keys(sd: Dict[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
    """Strip the wrapper prefix and drop non-encoder entries.

    Checkpoints saved from ``StreamformerForMultiTaskingSigLIP`` carry ``timesformer.`` (HF strips it via
    ``base_model_prefix``, modeling:1073; done by hand at downstream/OVIS/mask2former/
    timesformer_maskformer_model.py:123-124), plus ``task_heads.*`` / text-tower entries that
    ``extract_oad_feature.py:79-81`` drops."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in sd.items():
        if k.startswith("module."):
            k = k[len("module."):]
        if k.startswith("timesformer."):
            k = k[len("timesformer."):]
        elif k.split(".")[0] in ("task_heads", "text_encoder", "text_model", "logit_scale", "logit_bias"):
            continue
        out[k] = v
    return out


# ----------------------------------------------------------------------------------------------------------
# the module tree
# ----------------------------------------------------------------------------------------------------------
class _Node(nn.Module):
    """Parameter container with the reference's attribute path; numeric children index like ``nn.ModuleList``."""

    def _bind(self, root: "TimesformerMultiTaskingModelSigLIP") -> None:
        object.__setattr__(self, "_root_ref", weakref.ref(root))      # not a registered sub-module: no cycle

    def __getstate__(self):
        d = dict(self.__dict__)
        d.pop("_root_ref", None)              # weak references do not pickle; the root re-binds its tree in __setstate__
        return d

    @property
    def _root(self) -> "TimesformerMultiTaskingModelSigLIP":
        r = getattr(self, "_root_ref", None)
        r = r() if r is not None else None
        if r is None:
            raise RuntimeError("this sub-module is not attached to a TimesformerMultiTaskingModelSigLIP")
        return r

    def __getitem__(self, i: int) -> nn.Module:
        n = len(self)
        if isinstance(i, slice):
            return [self._modules[str(j)] for j in range(n)][i]
        if i < 0:
            i += n
        return self._modules[str(i)]

    def __len__(self) -> int:
        return sum(1 for k in self._modules if k.isdigit())

    def __bool__(self) -> bool:       # a module is truthy whatever __len__ says
        return True

    def __iter__(self):
        return (self._modules[str(j)] for j in range(len(self)))


def _staged_as(dtype: torch.dtype) -> Optional[int]:
    """The SF_* code a checkpoint dtype is staged in as it is (None: converted to fp32 first)."""
    return None if dtype == torch.uint8 else _TORCH2SF.get(dtype)


def _to_frame_major(x: torch.Tensor, T: int) -> torch.Tensor:
    """reference (B, N*T, D), token = n*T + t  ->  [B, T, N, D] contiguous fp32"""
    B, NT, D = x.shape
    return x.reshape(B, NT // T, T, D).permute(0, 2, 1, 3).contiguous().float()


def _to_patch_major(h: torch.Tensor) -> torch.Tensor:
    B, T, N, D = h.shape
    return h.permute(0, 2, 1, 3).reshape(B, N * T, D)


class TimesformerEmbeddingsSigLIP(_Node):
    """``model.embeddings(pixel_values) -> (B, N*T, D)`` (TimesformerEmbeddingsSigLIP.forward, modeling:413-457)."""

    def forward(self, pixel_values: torch.Tensor) -> torch.Tensor:
        m = self._root
        B, T, _, H, W = pixel_values.shape
        ws = m._stage_ws(B, T, H, W)
        dev = m.device
        x = pixel_values.to(dev)
        if x.dtype not in (torch.float32, torch.bfloat16, torch.uint8):
            x = x.float()
        x = x.contiguous()
        c = m.config
        N = (H // c.patch_size) * (W // c.patch_size)
        h = torch.empty(B, T, N, c.hidden_size, dtype=torch.float32, device=dev)
        pos = m._pos_table(H, W)
        nat.launch(dev, nat.lib.sf_embed, m._handle, x.data_ptr(), _TORCH2SF[x.dtype], B, T, H, W, h.data_ptr(), nat.ptr(pos), workspace=ws)
        return _to_patch_major(h)


class TimesformerLayerSigLIP(_Node):
    """``model.encoder.layer[i](hidden_states, T, output_attentions=False) -> (hidden_states[, attn])``
    (TimesformerLayerSigLIP.forward, modeling:934-1004), patch-major in and out."""

    index: int = 0

    def forward(self, hidden_states: torch.Tensor, T: int, output_attentions: bool = False):
        out = self._root.encoder._run(hidden_states, T, self.index, self.index + 1, output_attentions)
        return (out[0],) + ((out[1][0],) if output_attentions else ())


class TimesformerEncoder(_Node):
    """``model.encoder(hidden_states, num_frames=T, ...)`` (TimesformerEncoder.forward, modeling:1019-1063)."""

    def _run(self, hidden_states: torch.Tensor, T: int, la: int, lb: int, want_attn: bool):
        m = self._root
        B, NT, D = hidden_states.shape
        H, W = m._grid(NT, T)
        ws = m._stage_ws(B, T, H, W)
        dev = m.device
        h = _to_frame_major(hidden_states.to(dev), T)
        N = NT // T
        att = torch.empty(lb - la, B * T, m.config.num_attention_heads, N, N, dtype=torch.float32, device=dev) if want_attn else None
        nat.launch(dev, nat.lib.sf_layers, m._handle, h.data_ptr(), B, T, H, W, la, lb, nat.ptr(att), workspace=ws)
        return _to_patch_major(h), (tuple(att[i] for i in range(lb - la)) if want_attn else None)

    def forward(self, hidden_states: torch.Tensor, num_frames: int, output_attentions: bool = False,
                output_hidden_states: bool = False, return_dict: bool = True):
        L = self._root.config.num_hidden_layers
        hs, atts = ((hidden_states,) if output_hidden_states else None), (() if output_attentions else None)
        x = hidden_states
        if output_hidden_states:                      # layer by layer: every intermediate is an output
            for i in range(L):
                x, a = self._run(x, num_frames, i, i + 1, output_attentions)
                hs = hs + (x,)
                if output_attentions:
                    atts = atts + a
        else:
            x, a = self._run(x, num_frames, 0, L, output_attentions)
            atts = a
        if not return_dict:
            return tuple(v for v in (x, hs, atts) if v is not None)
        return ModelOutput(last_hidden_state=x, hidden_states=hs, attentions=atts)


class _PostLayerNorm(_Node):
    """nn.LayerNorm(D, eps) with the post_layernorm weights (modeling:1251, 1330), any leading shape."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        m = self._root
        m._sync()
        dev = m.device
        xf = x.to(dev, torch.float32).contiguous()
        y = torch.empty_like(xf)
        g = self.weight.detach().to(dev, torch.float32).contiguous()
        b = self.bias.detach().to(dev, torch.float32).contiguous()
        nat.launch(dev, nat.lib.sf_op_layernorm, xf.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), xf.numel() // xf.shape[-1], xf.shape[-1],
                   float(m.config.layer_norm_eps))
        return y


class TimesformerSiglipMultiheadAttentionPoolingHead(_Node):
    """TimesformerSiglipMultiheadAttentionPoolingHead.forward (modeling:1141-1154): x (F, N, D) -> (F, D)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        m = self._root
        Fr, N, D = x.shape
        H, W = m._grid(N, 1)
        ws = m._stage_ws(Fr, 1, H, W)
        dev = m.device
        xf = x.to(dev, torch.float32).contiguous()
        pool = torch.empty(Fr, D, dtype=torch.float32, device=dev)
        nat.launch(dev, nat.lib.sf_post_head, m._handle, xf.data_ptr(), Fr, 1, H, W, None, pool.data_ptr(), workspace=ws)
        return pool


_NODE_CLASSES = {"embeddings": TimesformerEmbeddingsSigLIP, "encoder": TimesformerEncoder, "post_layernorm": _PostLayerNorm,
                 "head": TimesformerSiglipMultiheadAttentionPoolingHead}


class TimesformerMultiTaskingModelSigLIP(nn.Module):
    """MI355X-native stand-in for the reference class of the same name (modeling:1241-1354)."""

    config_class = StreamformerConfig
    base_model_prefix = "timesformer"      # modeling:1073
    main_input_name = "pixel_values"       # modeling:1074

    def __init__(self, config: StreamformerConfig, compute_dtype: Any = "fp32", device: Any = None,
                 fuse_temporal_proj: bool = True):
        super().__init__()
        if config.attention_type != "divided_space_time":
            # the reference asserts the same wherever StreamFormer touches the encoder (modeling:1272-1274)
            raise NotImplementedError(
                f"attention_type={config.attention_type!r}: only 'divided_space_time' is on the StreamFormer path")
        if config.hidden_act not in _ACT_CODES:
            raise ValueError(f"unsupported hidden_act {config.hidden_act!r}")
        self._compute = nat.compute_mode(compute_dtype)
        self.config = config
        self._fuse = bool(fuse_temporal_proj)
        self._lora = bool(config.add_lora_spatial)
        # the packed handle, its token (device, version sum, ...) and one workspace per call shape
        self._native = nat.PackedHandle(self._create, nat.lib.sf_load_tensor, self._finalize, nat.lib.sf_destroy, "encoder", self._on_release,
                                        _staged_as, "the StreamFormer HIP encoder runs on an AMD GPU only: call .to('cuda') first "
                                        "(there is no CPU fallback)")
        self._force_repack = True
        self._pack_epoch = 0                # counts re-packs: a StreamSnapshot of this model remembers the one it was taken in
        self._pos_cache: Dict[tuple, torch.Tensor] = {}
        self._plist: List[torch.Tensor] = []
        from .processing import TimesformerImageProcessor
        self.image_processor = TimesformerImageProcessor(size=(config.image_size, config.image_size),
                                                         crop_size={"height": config.image_size, "width": config.image_size})
        self._build_tree()
        self._engine = None                 # autograd bridge state (autograd.TrainEngine), built on the first training forward
        # Constructed in eval mode, like a from_pretrained() model: the autograd path (12 GB of saved activations per 8
        # clips) is entered only after an explicit .train(), which every training loop issues (tools/finetune_tools.py:403).
        self.eval()
        if device is not None:
            self.to(device)

    # --------------------------------------------------------------------------------- parameter tree
    def _node_for(self, path: List[str]) -> _Node:
        """Get / create the container module at ``path`` (attribute names of the reference)."""
        node: nn.Module = self
        for depth, name in enumerate(path):
            child = node._modules.get(name)
            if child is None:
                if depth == 0:
                    cls = _NODE_CLASSES.get(name, _Node)
                elif depth == 2 and path[0] == "encoder" and path[1] == "layer":
                    cls = TimesformerLayerSigLIP
                else:
                    cls = _Node
                child = cls()
                child._bind(self)
                if cls is TimesformerLayerSigLIP:
                    child.index = int(name)
                node.add_module(name, child)
            node = child
        return node

    def _default_value(self, key: str, shape: Tuple[int, ...], g: torch.Generator) -> torch.Tensor:
        """Reference-like defaults for a freshly constructed model (modeling:1077-1109, :896, :377, :533-534):
        trunc-normal(0.02) matrices, zero biases, identity LayerNorm, zero gate / time embeddings, LoRA A ~ N(0, 0.02), B = 0."""
        std = float(self.config.initializer_range)
        if key.endswith("layernorm.weight") or key.endswith("layernorm_before.weight") or key.endswith("layernorm_after.weight"):
            return torch.ones(shape)
        if key.endswith(".bias") or key.endswith("gating") or key.endswith("time_embeddings") or key.endswith("_lora_b.weight"):
            return torch.zeros(shape)
        if key == "head.probe":
            return torch.randn(shape, generator=g)
        if key.endswith("_lora_a.weight"):
            return torch.randn(shape, generator=g) * 0.02
        return torch.nn.init.trunc_normal_(torch.empty(shape), std=std, a=-2 * std, b=2 * std, generator=g)

    def _register(self, key: str, value: torch.Tensor, like: Optional[torch.Tensor] = None) -> None:
        *path, leaf = key.split(".")
        node = self._node_for(path)
        if like is not None:
            value = value.to(device=like.device, dtype=like.dtype)
        node.register_parameter(leaf, nn.Parameter(value))

    def _build_tree(self) -> None:
        g = torch.Generator().manual_seed(0)
        c = self.config
        for k, shape in expected_keys(c, self._lora).items():
            self._register(k, self._default_value(k, shape, g))
        for i in range(c.num_hidden_layers):      # persistent buffer of the reference, unused by its forward (modeling:515-517)
            self._node_for(["encoder", "layer", str(i), "temporal_attention", "attention"]).register_buffer(
                "mask", torch.tril(torch.ones(c.num_frames, c.num_frames)))
        self._refresh_plist()

    def _refresh_plist(self) -> None:
        self._named = OrderedDict(self.named_parameters())
        self._plist = list(self._named.values())
        self._force_repack = True

    def _param(self, key: str) -> torch.Tensor:
        return self._named[key]

    # ------------------------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True, assign: bool = False):
        """``nn.Module.load_state_dict`` after key normalisation: wrapper (``timesformer.``) / DDP (``module.``) prefixes
        stripped, task-head and text-tower entries dropped, LoRA factors adopted when the checkpoint has them."""
        sd = normalize_checkpoint_keys(state_dict)
        if any("_lora_" in k for k in sd) and not self._lora:
            self._enable_lora_keys()
        exp = expected_keys(self.config, self._lora)
        for k, shape in exp.items():
            if k in sd and tuple(sd[k].shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shape)}")
        mask_shape = (self.config.num_frames,) * 2
        sd = OrderedDict((k, v) for k, v in sd.items()
                         if not (k.endswith("temporal_attention.attention.mask") and tuple(v.shape) != mask_shape))
        res = super().load_state_dict(sd, strict=False, assign=assign)
        missing = [k for k in res.missing_keys if not k.endswith("temporal_attention.attention.mask")]   # constant buffers
        unexpected = list(res.unexpected_keys)
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:8]}{'...' if len(missing) > 8 else ''}, "
                               f"unexpected {unexpected[:8]}{'...' if len(unexpected) > 8 else ''}")
        if assign:
            self._refresh_plist()
        self._force_repack = True
        from torch.nn.modules.module import _IncompatibleKeys      # what nn.Module.load_state_dict returns (also unpacks as a pair)
        return _IncompatibleKeys(missing, unexpected)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, *model_args, config: Optional[StreamformerConfig] = None,
                        compute_dtype: Any = "fp32", device: Any = None, device_map: Any = None,
                        torch_dtype: Any = None, **kwargs):
        path = str(pretrained_model_name_or_path)
        if not os.path.isdir(path):
            # a hub id ("org/name"), as the reference's HF classmethod takes it (modeling:1066-1075): resolve it to a local snapshot through
            # huggingface_hub (cache first, then the network); every failure — no network, no such repo, library absent — names the fix
            try:
                from huggingface_hub import snapshot_download
                path = snapshot_download(repo_id=path, revision=kwargs.pop("revision", None), cache_dir=kwargs.pop("cache_dir", None),
                                         local_files_only=bool(kwargs.pop("local_files_only", False)),
                                         allow_patterns=["config.json", "*.safetensors", "pytorch_model.bin", "model.bin"])
            except Exception as e:
                raise OSError(f"{pretrained_model_name_or_path!r} is not a local directory and could not be fetched from the hub "
                              f"({type(e).__name__}: {e}).  Download the checkpoint (config.json + model.safetensors or pytorch_model.bin) "
                              "and pass its directory") from e
        cfg_over = {k: kwargs.pop(k) for k in list(kwargs) if k in StreamformerConfig().to_dict()}
        cfg = config or StreamformerConfig.from_pretrained(path, **cfg_over)
        from .convert import read_state_dict      # (convert imports this module)
        sd = read_state_dict(path, ("model.safetensors", "pytorch_model.bin", "model.bin"))
        if isinstance(sd, dict) and "model" in sd and "state_dict" not in sd and not any(k.startswith(("embeddings", "timesformer")) for k in sd):
            sd = sd["model"]     # checkpoint-*.pth layout (utils.py:625-631)
        if any("_lora_" in k for k in sd):
            cfg.add_lora_spatial = True
        model = cls(cfg, compute_dtype=compute_dtype)
        model.load_state_dict(sd, strict=True)
        if isinstance(torch_dtype, torch.dtype):
            model.to(torch_dtype)
        if device is None and isinstance(device_map, (str, int, torch.device)):
            device = device_map
        if device is None and torch.cuda.is_available():
            device = "cuda"
        if device is not None:
            model.to(device)
        model.eval()
        return model

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True) -> None:
        os.makedirs(save_directory, exist_ok=True)
        self.config.add_lora_spatial = self._lora
        self.config.save_pretrained(save_directory)
        from .convert import write_state_dict
        write_state_dict(save_directory, self.state_dict(), "model.safetensors" if safe_serialization else "pytorch_model.bin", safe_serialization)

    # ------------------------------------------------------------------------------ LoRA surface
    def _enable_lora_keys(self) -> None:
        if self._lora:
            return
        self._lora = True
        self.config.add_lora_spatial = True
        g = torch.Generator().manual_seed(1)
        like = self._plist[0]
        for i in range(self.config.num_hidden_layers):
            for k, shape in _lora_keys(self.config, i).items():
                self._register(k, self._default_value(k, shape, g), like=like)
        self._refresh_plist()

    def add_lora_spatial(self) -> None:
        """modeling:1271-1282: rank-32 LoRA on every spatial qkv / output.dense; base weights frozen."""
        self._enable_lora_keys()
        for i in range(self.config.num_hidden_layers):
            for n in ("attention.attention.qkv", "attention.output.dense"):
                for leaf in ("weight", "bias"):
                    p = self._named.get(f"encoder.layer.{i}.{n}.{leaf}")
                    if p is not None:
                        p.requires_grad = False
        print("Added LoRA to the following layers: ",
              [f"timesformer.encoder.layer.{i}.attention" for i in range(self.config.num_hidden_layers)])

    def frozen_spatial(self) -> None:
        """modeling:1284-1297 freezes the spatial qkv (its ``attention.dense`` line would raise in the
        reference; only the qkv freeze is observable)."""
        for i in range(self.config.num_hidden_layers):
            for leaf in ("weight", "bias"):
                p = self._named.get(f"encoder.layer.{i}.attention.attention.qkv.{leaf}")
                if p is not None:
                    p.requires_grad = False

    def trainable_parameter_names(self) -> List[str]:
        return [k for k, p in self._named.items() if p.requires_grad]

    # ------------------------------------------------------------------------- module-like surface
    @property
    def device(self) -> torch.device:
        return self._plist[0].device

    @property
    def dtype(self) -> torch.dtype:
        return self._plist[0].dtype

    @property
    def compute_dtype(self) -> str:
        return "bf16" if self._compute == nat.SF_COMPUTE_BF16 else "bf16x3"

    def num_parameters(self) -> int:
        return sum(v.numel() for v in self._plist)

    def _train_engine(self):
        """The flat-buffer training state behind the autograd bridge; rebuilt when device / LoRA / freeze pattern change."""
        from .autograd import TrainEngine
        if self._engine is None or self._engine.signature != TrainEngine._signature(self):
            self._engine = None
            self._engine = TrainEngine(self)
        return self._engine

    def _apply(self, fn, recurse: bool = True):
        out = super()._apply(fn, recurse)
        self._refresh_plist()            # .to() / .cuda() / .half(): new storage -> re-pack, drop device-bound scratch
        self._engine = None
        self._native.workspaces.clear()
        self._pos_cache.clear()
        return out

    def set_compute_dtype(self, compute_dtype: Any):
        c = nat.compute_mode(compute_dtype)
        if c != self._compute:
            self._compute = c
            self._force_repack = True
            self._native.workspaces.clear()
        return self

    def refresh_weights(self) -> None:
        """Force a re-pack of the library's operands on the next forward (needed only after writes the version counters
        cannot see, e.g. through ``param.data``)."""
        self._force_repack = True

    # -------------------------------------------------------------------- copy / pickle (torch.save(model), copy.deepcopy)
    def __getstate__(self):
        d = dict(self.__dict__)               # (_native copies as an empty owner: native state is rebuilt from the parameters on first use)
        d["_force_repack"] = True
        d["_pos_cache"] = {}
        d["_engine"] = None
        d.pop("_named", None)
        d.pop("_plist", None)
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        for m in self.modules():
            if isinstance(m, _Node):
                m._bind(self)
        self._refresh_plist()

    # ------------------------------------------------------------------------------ native sync
    def _sf_config(self) -> nat.SfConfig:
        c = self.config
        return nat.SfConfig(c.image_size, c.patch_size, c.num_channels, c.num_frames, c.hidden_size,
                            c.num_hidden_layers, c.num_attention_heads, c.intermediate_size,
                            _ACT_CODES[c.hidden_act], int(bool(c.qkv_bias)), int(bool(c.enable_causal_temporal)),
                            int(self._lora), float(c.layer_norm_eps))

    def _token(self):
        v = 0
        for p in self._plist:
            v += p._version
        ip = self.image_processor
        return (self._plist[0].device, self._compute, v, tuple(ip.image_mean), tuple(ip.image_std), ip.rescale_factor)

    @property
    def _handle(self):
        return self._native.handles.get(None)

    def _create(self, device_index: int):
        h = nat.C.c_void_p()
        nat.check(nat.lib.sf_create(nat.C.byref(self._sf_config()), device_index, nat.C.byref(h)))
        return h

    def _finalize(self, h) -> None:
        nat.check(nat.lib.sf_finalize_weights(h, self._compute, 1, int(self._fuse)))
        ip = self.image_processor           # uint8 frames: rescale + normalize fused into the patch kernel
        nch = len(ip.image_mean)
        mean = (nat.C.c_float * nch)(*ip.image_mean)
        std = (nat.C.c_float * nch)(*ip.image_std)
        nat.check(nat.lib.sf_set_pixel_normalization(h, mean, std, nch, ip.rescale_factor))

    def _on_release(self) -> None:
        """A packing goes (its live StreamCaches with it: PackedHandle.dependents).  Only where one was held: before the first handle
        there is no snapshot to age and no position table to drop."""
        self._pack_epoch += 1            # the snapshots taken from its caches are stale
        self._pos_cache.clear()

    def _sync(self, trust_versions: bool = False) -> None:
        """Create the handle on the current device and (re)upload packed weights when stale.
        ``trust_versions``: skip the scan of the parameters' version counters (~45 us for SigLIP-base) — used for the
        frames of a running stream, whose valid cache already proves the packing it was started on is still the live one."""
        native = self._native
        if trust_versions and native.handles and not self._force_repack:
            return
        tok = self._token()
        if self._force_repack:
            native.token = None          # whatever is packed is stale
        native.get(tok[0], tok, self._named.items)
        self._force_repack = False

    def _pos_table(self, H: int, W: int) -> Optional[torch.Tensor]:
        """Resized position table for non-native inputs (modeling:380-411): a handful of KFLOP of
        bicubic-antialias resampling done once per resolution with torch on the host."""
        c = self.config
        N = c.num_patches
        if (H // c.patch_size) * (W // c.patch_size) == N and H == W:
            return None
        key = (H, W)
        if key not in self._pos_cache:
            M = int(round(N ** 0.5))
            assert N == M * M
            w0, h0 = W // c.patch_size, H // c.patch_size
            pe = self._param("embeddings.position_embeddings").detach().to("cpu", torch.float32)
            pe = pe.reshape(1, M, M, c.hidden_size).permute(0, 3, 1, 2)
            pe = F.interpolate(pe, size=(w0, h0), mode="bicubic", antialias=True)
            assert (w0, h0) == tuple(pe.shape[-2:])
            self._pos_cache[key] = pe.permute(0, 2, 3, 1).reshape(-1, c.hidden_size).contiguous().to(self.device)
        return self._pos_cache[key]

    # ------------------------------------------------------------------------------------ forward
    def new_cache(self, batch_size: int = 1, max_frames: Optional[int] = None, height: Optional[int] = None,
                  width: Optional[int] = None, policy: str = "stop") -> StreamCache:
        """``policy="slide"``: bounded memory for streams that outlive the cache — past ``max_frames`` every new frame replaces the
        oldest one and attends to the last ``max_frames`` frames (an extension: the reference raises at ``config.num_frames``,
        timesformer_encoder.py:343-348)."""
        self._sync()
        c = self.config
        with torch.cuda.device(self.device):
            return StreamCache(self, batch_size, max_frames or c.num_frames, height or c.image_size, width or c.image_size, policy)

    def forward(self, pixel_values: torch.Tensor, output_attentions: Optional[bool] = None,
                output_hidden_states: Optional[bool] = None, return_dict: Optional[bool] = None,
                past_key_values: Optional[StreamCache] = None, use_cache: bool = False,
                cache_position: Optional[torch.Tensor] = None, stream_ids: Optional[Sequence[int]] = None):
        """``stream_ids`` (with ``past_key_values``): row ``i`` of ``pixel_values`` is the next frame of stream ``stream_ids[i]`` of a
        batched cache; any subset of its streams, each continuing from its own position, outputs in the same order.  Several
        frames per call (``T > 1``) are the prefill of one stream."""
        c = self.config
        output_attentions = c.output_attentions if output_attentions is None else output_attentions
        output_hidden_states = c.output_hidden_states if output_hidden_states is None else output_hidden_states
        return_dict = c.use_return_dict if return_dict is None else return_dict
        if pixel_values.dim() != 5:
            raise ValueError(f"pixel_values must be (B, T, C, H, W), got {tuple(pixel_values.shape)}")
        B, T, C_, H, W = pixel_values.shape
        if C_ != c.num_channels:
            raise ValueError(f"expected {c.num_channels} channels, got {C_}")
        streaming = bool(use_cache) or past_key_values is not None
        if stream_ids is not None:
            if not isinstance(past_key_values, StreamCache):
                raise ValueError("stream_ids names streams of a batched cache: pass past_key_values=model.new_cache(batch_size=...)")
            if output_attentions or output_hidden_states:
                raise NotImplementedError("output_attentions / output_hidden_states are not available together with stream_ids: "
                                          "use a lockstep call (all streams, no stream_ids) for them")
            stream_ids = [int(i) for i in stream_ids]
            if len(stream_ids) != B:
                raise ValueError(f"pixel_values carries {B} streams but stream_ids names {len(stream_ids)}")
        if self.training and torch.is_grad_enabled() and not streaming and any(p.requires_grad for p in self._plist):
            # the reference wrapper's training forward (modeling:1506-1511): outputs carry a grad_fn (autograd.py)
            if output_attentions or output_hidden_states:
                raise NotImplementedError("output_attentions / output_hidden_states are not available on the autograd path: "
                                          "call under torch.no_grad() or in eval mode for them")
            if self.device.type != "cuda":
                raise RuntimeError("the StreamFormer HIP encoder runs on an AMD GPU only: call .to('cuda') first")
            from .autograd import encoder_forward_with_grad
            x = pixel_values.to(self.device)
            lhs, pool = encoder_forward_with_grad(self, x)
            if not return_dict:
                return (lhs,)
            return BaseModelOutputWithPooling(lhs, pool)
        self._sync(trust_versions=isinstance(past_key_values, StreamCache) and past_key_values.valid
                   and past_key_values.get_seq_length() > 0)
        dev = self.device
        x = pixel_values.to(dev)
        if x.dtype not in (torch.float32, torch.bfloat16, torch.uint8):
            x = x.float()
        if x.dtype == torch.uint8 and W % 8:
            x = self.image_processor.normalize(x)       # byte path needs 8-pixel rows; fall back to fp32 frames
        x = x.contiguous()
        N = (H // c.patch_size) * (W // c.patch_size)
        D, L = c.hidden_size, c.num_hidden_layers
        pos = self._pos_table(H, W)
        out_dtype = self.dtype if self.dtype in (torch.bfloat16, torch.float16) else None    # a half-precision module answers in kind

        def cast(t):
            return t if (t is None or out_dtype is None) else t.to(out_dtype)

        with torch.cuda.device(dev):
            skey = int(nat.current_stream_handle(dev) or 0)          # one workspace per HIP stream: concurrent forwards never share scratch
            lhs = torch.empty(B, T, N, D, dtype=torch.float32, device=dev)
            pool = torch.empty(B, T, D, dtype=torch.float32, device=dev)
            hs = torch.empty(L + 1, B, T, N, D, dtype=torch.float32, device=dev) if output_hidden_states else None
            # spatial probabilities per layer, of the new frames when streaming (timesformer_encoder.py:494, 557, 720-754); the
            # reference materialises these anyway (modeling:703-705), here only on request
            att = torch.empty(L, B * T, c.num_attention_heads, N, N, dtype=torch.float32, device=dev) if output_attentions else None
            if streaming:
                cache = self._forward_stream(x, pos, past_key_values, cache_position, stream_ids, lhs, pool, hs, att, skey)
            else:
                h = self._native.handles[None]
                ws = self._native.workspace(nat.sized(nat.lib.sf_workspace_bytes, h, B, T, H, W), dev, ("f", B, T, H, W, skey))
                if att is not None:
                    nat.launch(dev, nat.lib.sf_forward_attentions, h, x.data_ptr(), _TORCH2SF[x.dtype], B, T, H, W, lhs.data_ptr(), pool.data_ptr(),
                               nat.ptr(hs), att.data_ptr(), nat.ptr(pos), workspace=ws)
                else:
                    nat.launch(dev, nat.lib.sf_forward, h, x.data_ptr(), _TORCH2SF[x.dtype], B, T, H, W, lhs.data_ptr(), pool.data_ptr(), nat.ptr(hs),
                               nat.ptr(pos), workspace=ws)
        hidden = None
        if hs is not None:
            # the reference hands back patch-major (B, N*T, D) tensors (modeling:1352): permuted views
            hidden = tuple(cast(hs[i]).permute(0, 2, 1, 3).reshape(B, N * T, D) for i in range(L + 1))
        lhs, pool = cast(lhs), cast(pool)
        attentions = tuple(att[i] for i in range(L)) if att is not None else None
        if streaming:
            return self._stream_output(lhs, pool, hidden, attentions, cache, use_cache or past_key_values is not None, return_dict)
        if not return_dict:
            return (lhs,) + ((hidden,) if hidden is not None else ()) + ((attentions,) if attentions is not None else ())
        return BaseModelOutputWithPooling(lhs, pool, hidden_states=hidden, attentions=attentions)

    def _forward_stream(self, x, pos, cache, cache_position, stream_ids, lhs, pool, hs, att, skey):
        """One streaming call into the caller's output tensors: every stream of ``cache`` in lockstep, or the streams that
        ``stream_ids`` names.  Returns the cache (a new one when the caller passed none)."""
        B, T, _, H, W = x.shape
        ragged = stream_ids is not None
        if cache is None:
            cache = StreamCache(self, B, max(self.config.num_frames, T), H, W)
        elif not isinstance(cache, StreamCache):
            raise TypeError("past_key_values must be the StreamCache a previous call returned (or model.new_cache())")
        ch = cache._require()
        if cache._model() is not self:
            raise ValueError("past_key_values belongs to another model")
        # a sliding-window cache saturates get_seq_length() at its capacity while frames_seen keeps counting: an HF-style
        # caller that derives cache_position from get_seq_length() is as right as one that counts frames
        if ragged and cache_position is not None:
            # one start position per named stream ([B] or [B, T]); checked for the ids the library will accept
            cp = torch.as_tensor(cache_position)
            cp = (cp[:, 0] if cp.dim() == 2 else cp.reshape(-1)).tolist()
            if len(cp) != B:
                raise ValueError(f"cache_position must give one start position per named stream ({B}), got {len(cp)}")
            seen = cache.frames_seen_per_stream
            for sid, pos0 in zip(stream_ids, cp):
                if 0 <= sid < cache.batch and int(pos0) not in (seen[sid], min(seen[sid], cache.max_frames)):
                    raise ValueError(f"cache_position {int(pos0)} does not continue stream {sid} ({seen[sid]} frames seen)")
        elif cache_position is not None and int(cache_position[0]) not in (cache.frames_seen, cache.get_seq_length()):
            raise ValueError("cache_position must continue the cache (vqa_enc:1340-1349)")
        if ragged and (cache.H, cache.W) != (H, W):
            raise ValueError("past_key_values was created for a different resolution")
        if not ragged and (cache.batch, cache.H, cache.W) != (B, H, W):
            raise ValueError("past_key_values was created for a different batch size / resolution")
        h = self._native.handles[None]
        # (a lockstep call has B == cache.batch)
        ws = self._native.workspace(nat.sized(nat.lib.sf_stream_workspace_bytes, h, ch, T), x.device, ("s", cache.batch, T, H, W, skey))
        frames = (h, ch, x.data_ptr(), _TORCH2SF[x.dtype], T)
        if ragged:
            nat.launch(x.device, nat.lib.sf_forward_stream_slots, *frames, nat.i32_array(stream_ids), B, lhs.data_ptr(), pool.data_ptr(), nat.ptr(pos),
                       workspace=ws)
        elif att is not None:
            nat.launch(x.device, nat.lib.sf_forward_stream_attentions, *frames, lhs.data_ptr(), pool.data_ptr(), nat.ptr(hs), att.data_ptr(),
                       nat.ptr(pos), workspace=ws)
        else:
            nat.launch(x.device, nat.lib.sf_forward_stream, *frames, lhs.data_ptr(), pool.data_ptr(), nat.ptr(hs), nat.ptr(pos), workspace=ws)
        return cache

    @staticmethod
    def _stream_output(lhs, pool, hidden, attentions, cache, keep_cache, return_dict):
        if not return_dict:
            return (lhs,) + ((hidden,) if hidden is not None else ()) + ((attentions,) if attentions is not None else ()) + (cache,)
        return BaseModelOutputWithPast(lhs, past_key_values=cache if keep_cache else None,
                                       hidden_states=hidden, attentions=attentions, pooler_output=pool)

    # -------------------------------------------------------------------------------- sub-modules
    # The reference's users that drive the encoder piecewise (ViT-Adapter interaction blocks:
    # `blk(x, T, output_attentions=False)[0]`, modeling_timesformer_siglip_adapter.py:424-425; the video
    # classifier: embeddings -> encoder -> post_layernorm -> head, downstream/AR/...:121-134) keep their
    # call shapes: tensors cross this surface in the reference's PATCH-major (B, N*T, D) order and are
    # permuted to the library's frame-major layout around each native call.
    def _stage_ws(self, B: int, T: int, H: int, W: int):
        self._sync()
        return self._native.workspace(nat.sized(nat.lib.sf_workspace_bytes, self._handle, B, T, H, W), self.device,
                                      ("f", B, T, H, W, int(nat.current_stream_handle(self.device) or 0)))

    def _grid(self, n_tokens: int, T: int) -> Tuple[int, int]:
        """(H, W) of a frame whose patch grid has n_tokens / T cells (square, or the config's aspect)."""
        N = n_tokens // T
        P = self.config.patch_size
        side = int(round(N ** 0.5))
        if side * side != N or N * T != n_tokens:
            raise ValueError(f"{n_tokens} tokens do not form {T} frames of a square patch grid")
        return side * P, side * P

    @torch.no_grad()
    def forward_features(self, pixel_values: torch.Tensor, pooling_method: str = "mean") -> torch.Tensor:
        """StreamformerForMultiTaskingSigLIP.forward_features (modeling:1525-1536): "mean" over frames (the default),
        "no_pooling" = every frame's pooled feature, anything else = the last frame."""
        pooled = self(pixel_values).pooler_output
        if pooling_method == "mean":
            return torch.mean(pooled, 1, False)
        if pooling_method == "no_pooling":
            return pooled
        return pooled[:, -1]


class TimesformerVisionTower(nn.Module):
    """The VideoQA vision tower (vqa_enc:1462-1598): ctor ``(vision_tower, vision_tower_cfg, delay_load)``, ``load_model``,
    the per-stream state machine (``past_key_values`` threaded through calls, outputs concatenated along time, the last
    ``context_length`` frames returned, ``clear_cache()``) and the read-only properties LLaVA reads.

    ``vision_tower`` is a checkpoint directory (``from_pretrained``) or an already constructed encoder;
    ``vision_tower_cfg`` any object with the reference's optional attributes (``streaming_mode``, ``context_length``,
    ``unfreeze_mm_vision_tower``, ``mm_tunable_parts``) — keyword arguments override it.  Memory is bounded: only the
    window that can still be returned is kept (the reference keeps every frame it has ever seen)."""

    def __init__(self, vision_tower, vision_tower_cfg: Any = None, delay_load: bool = False, *, context_length: Optional[int] = None,
                 streaming_mode: Optional[bool] = None, max_frames: Optional[int] = None, compute_dtype: Any = "fp32",
                 cache_policy: str = "stop"):
        super().__init__()
        self.is_loaded = False
        self._compute_dtype = compute_dtype
        self._max_frames = max_frames
        self._cache_policy = cache_policy        # "slide": streams may outlive max_frames / config.num_frames (StreamCache policy)
        if isinstance(vision_tower, nn.Module):
            self.vision_tower_name = getattr(vision_tower, "name_or_path", type(vision_tower).__name__)
            self._adopt(vision_tower)
        else:
            self.vision_tower_name = str(vision_tower)
            # vqa_enc:1472-1492: every branch ends in load_model() ("Force loading checkpoint!!!"), delay_load included
            self.load_model()
        cfg = vision_tower_cfg
        self.streaming_mode = bool(getattr(cfg, "streaming_mode", False) if streaming_mode is None else streaming_mode)
        if self.streaming_mode:
            self.context_length = int(getattr(cfg, "context_length", 16) if context_length is None else context_length)
            self.past_key_values: Optional[StreamCache] = None
            self.hidden_states: Optional[torch.Tensor] = None
            self.new_frame_features: Optional[torch.Tensor] = None      # (B, T_new, N, D) of the last call alone (read-only: the window is not re-sliced)
        self._spare: Optional[StreamCache] = None

    def _adopt(self, model: TimesformerMultiTaskingModelSigLIP) -> None:
        self.vision_tower = model
        self.config = model.config
        # vqa_enc:1515-1521 builds a processor of the model's size; the encoder already owns exactly that one, and its
        # mean / std are what the fused uint8 path applies
        self.image_processor = model.image_processor
        self.vision_tower.requires_grad_(False)
        self.is_loaded = True

    def load_model(self, device_map=None) -> None:
        if self.is_loaded:
            print("{} is already loaded, `load_model` called again, skipping.".format(self.vision_tower_name))
            return
        self._adopt(TimesformerMultiTaskingModelSigLIP.from_pretrained(self.vision_tower_name, device_map=device_map,
                                                                         compute_dtype=self._compute_dtype))

    def clear_cache(self) -> None:
        """vqa_enc:1528-1530.  The K/V buffers are kept aside and recycled by the next stream instead of re-allocated."""
        if not self.streaming_mode:
            return
        self.hidden_states = None
        self.new_frame_features = None
        if self.past_key_values is not None and self.past_key_values.valid:
            self._spare = self.past_key_values
        self.past_key_values = None

    def _cache_for(self, B: int, H: int, W: int) -> StreamCache:
        pkv = self.past_key_values
        if pkv is not None and not pkv.valid:       # the model re-packed its weights: the old stream is gone
            pkv, self.past_key_values, self.hidden_states = None, None, None
        if pkv is None:
            sp, self._spare = self._spare, None
            if sp is not None and sp.valid and (sp.batch, sp.H, sp.W, sp.policy) == (B, H, W, self._cache_policy) and sp._model() is self.vision_tower:
                sp.reset()
                pkv = sp
            else:
                pkv = self.vision_tower.new_cache(B, self._max_frames or self.config.num_frames, H, W, policy=self._cache_policy)
        return pkv

    def forward(self, images):
        if self.streaming_mode:
            # images: the new frames of one stream, (1, T, C, H, W)   (vqa_enc:1532-1544)
            B, T, _, H, W = images.shape
            cache = self._cache_for(B, H, W)
            x = images if images.dtype == torch.uint8 else images.to(device=self.device, dtype=self.dtype)
            outputs = self.vision_tower(x, use_cache=True, past_key_values=cache, cache_position=None)
            self.past_key_values = outputs.past_key_values
            lhs = outputs.last_hidden_state
            self.new_frame_features = lhs
            self.hidden_states = lhs if self.hidden_states is None else torch.cat([self.hidden_states, lhs], dim=1)
            self.hidden_states = self.hidden_states[:, -self.context_length:]       # bounded: nothing older is ever returned
            return self.hidden_states.to(images.dtype if images.dtype.is_floating_point else lhs.dtype)
        if type(images) is list:
            # vqa_enc:1545-1555 (whose `image_features.shape` assert on a list cannot run): per item the last encoder
            # hidden state, patch-major (1, N*T, D), for a clip [T, C, H, W]
            feats = []
            for image in images:
                out = self.vision_tower(image.to(device=self.device, dtype=self.dtype).unsqueeze(0), output_hidden_states=True)
                feats.append(out.hidden_states[-1].to(image.dtype))
            return feats
        out = self.vision_tower(images.to(device=self.device, dtype=self.dtype), output_hidden_states=False)
        return out.last_hidden_state.to(images.dtype)        # (B, T, N, D)

    @property
    def dummy_feature(self):
        return torch.zeros(1, self.hidden_size, device=self.device, dtype=self.dtype)

    @property
    def dtype(self):
        for p in self.vision_tower.parameters():
            return p.dtype

    @property
    def device(self):
        for p in self.vision_tower.parameters():
            return p.device

    @property
    def hidden_size(self):
        return self.config.hidden_size

    @property
    def num_patches(self):
        return (self.config.image_size // self.config.patch_size) ** 2

    @property
    def num_patches_per_side(self):
        return self.config.image_size // self.config.patch_size

    @property
    def image_size(self):
        return self.config.image_size
