"""Online action detection: the reference's streaming LSTR detector (``downstream/OAD``, ``LSTRStream.stream_inference``) on the HIP
library, next to the streaming encoder.

``OnlineActionDetector`` holds the reference's parameter tree under the reference's names (``load_state_dict`` of a checkpoint's
``model_state_dict`` works) and runs ``csrc/sf_oad.hip``: per stream a device-resident ring of projected long-memory rows and the cached
compressed memory, several independent streams per call.  ``StreamingActionDetector`` couples it to the streaming encoder: one frame
in, the newest frame's class probabilities out.  Inference only; there is no fallback to torch.

Not built, and refused with ``NotImplementedError`` naming the field: the batch ``forward`` (top-k "knn" attention), ``FUTURE_*`` /
``ANTICIPATION_*`` / CCI generation (their tensors in a checkpoint are ignored and listed in ``ignored_keys``), the ``motion`` /
``twostream`` modalities, the ``EK100`` verb / noun classifiers, training, snapshots of the detector state.
"""
from __future__ import annotations

import bisect
import ctypes as C
import math
from collections import deque
from dataclasses import dataclass, field, asdict
from typing import Any, Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _native as nat

_ACT = {"gelu": 0, "relu": 2}
_IGNORED_PREFIXES = ("gen_query.", "gen_layer.", "final_query.", "work_fusions.", "fut_fusions.")
PE_MAX_LEN = 5000
FEATURE_SIZES = {"rgb_anet_resnet50": 2048, "rgb_kinetics_bninception": 1024, "rgb_kinetics_resnet50": 2048,
                 "streamformer_multitask_feature": 768, "streamformer_multitask_feature_so400m": 1152}


def _get(node: Any, path: str, default: Any = None) -> Any:
    for part in path.split("."):
        if node is None:
            return default
        node = node.get(part) if isinstance(node, dict) else getattr(node, part, None)
    return default if node is None else node


@dataclass
class OADConfig:
    """The reference's fields (``cfg.MODEL.LSTR.*``, ``cfg.INPUT.*``, ``cfg.DATA.*``, ``cfg.MODEL.FEATURE_HEAD.*``), flat."""
    VISUAL_SIZE: int = 768                       # FEATURE_SIZES[INPUT.VISUAL_FEATURE]
    MODALITY: str = "visual"
    DATA_NAME: str = "THUMOS"
    NUM_CLASSES: int = 22
    LINEAR_ENABLED: bool = True
    LINEAR_OUT_FEATURES: int = 1024
    NUM_HEADS: int = 4
    DIM_FEEDFORWARD: int = 1024
    ACTIVATION: str = "relu"
    LONG_MEMORY_NUM_SAMPLES: int = 64
    WORK_MEMORY_NUM_SAMPLES: int = 32
    ENC_MODULE: List[List[Any]] = field(default_factory=lambda: [[16, 1, True], [32, 2, True]])
    DEC_MODULE: List[Any] = field(default_factory=lambda: [-1, 2, True])
    FUTURE_SECONDS: int = 0
    FUTURE_NUM_SAMPLES: int = 0
    ANTICIPATION_SECONDS: int = 0
    ANTICIPATION_NUM_SAMPLES: int = 0

    def __post_init__(self):
        self.ENC_MODULE = [list(m) for m in self.ENC_MODULE]
        self.DEC_MODULE = list(self.DEC_MODULE)
        if self.MODALITY not in ("visual", "motion", "twostream"):
            raise ValueError(f"Unknown modality of {self.MODALITY}")
        if self.MODALITY != "visual":
            raise NotImplementedError(f"INPUT.MODALITY = {self.MODALITY!r}: the native detector takes the 'visual' features of the encoder only")
        if self.DATA_NAME == "EK100":
            raise NotImplementedError("DATA.DATA_NAME = 'EK100': the verb / noun classifiers are not part of the native detector")
        if self.ACTIVATION not in _ACT:
            raise ValueError(f"MODEL.LSTR.ACTIVATION should be relu/gelu, not {self.ACTIVATION}")
        if self.LONG_MEMORY_NUM_SAMPLES < 1:
            raise ValueError("MODEL.LSTR.LONG_MEMORY_NUM_SAMPLES: long-term memory cannot be empty for stream inference")
        if self.WORK_MEMORY_NUM_SAMPLES < 1:
            raise ValueError("MODEL.LSTR.WORK_MEMORY_NUM_SAMPLES must be positive")
        if not self.ENC_MODULE:
            raise ValueError("MODEL.LSTR.ENC_MODULE: the LSTR encoder cannot be disabled for stream inference")
        if len(self.ENC_MODULE) > 8:
            raise ValueError("MODEL.LSTR.ENC_MODULE: at most 8 modules")
        for m in self.ENC_MODULE:
            if len(m) != 3 or (m[0] != -1 and m[0] < 1) or m[1] < 1:
                raise ValueError(f"MODEL.LSTR.ENC_MODULE entry {m}: [queries | -1, layers, norm]")
        if self.ENC_MODULE[0][0] == -1:
            raise ValueError("MODEL.LSTR.ENC_MODULE[0] needs queries: stream inference compresses the long memory with them")
        if self.ENC_MODULE[0][1] != 1:
            raise ValueError("MODEL.LSTR.ENC_MODULE[0]: number of layers cannot be larger than 1 for stream inference")
        if len(self.DEC_MODULE) != 3 or self.DEC_MODULE[1] < 1:
            raise ValueError(f"MODEL.LSTR.DEC_MODULE {self.DEC_MODULE}: [-1, layers, norm]")
        if self.d_model % self.NUM_HEADS:
            raise ValueError("embed_dim must be divisible by num_heads")

    @property
    def d_model(self) -> int:
        if self.LINEAR_ENABLED and self.LINEAR_OUT_FEATURES != -1:
            return int(self.LINEAR_OUT_FEATURES)
        return int(self.VISUAL_SIZE)

    @property
    def generation_enabled(self) -> Optional[str]:
        """The first FUTURE_* / ANTICIPATION_* field that asks for what the native detector does not compute, or None."""
        for k in ("FUTURE_SECONDS", "FUTURE_NUM_SAMPLES", "ANTICIPATION_SECONDS", "ANTICIPATION_NUM_SAMPLES"):
            if getattr(self, k) > 0:
                return k
        return None

    def to_reference_dict(self) -> Dict[str, Any]:
        d = asdict(self)
        lstr = {k: d[k] for k in ("NUM_HEADS", "DIM_FEEDFORWARD", "ACTIVATION", "LONG_MEMORY_NUM_SAMPLES", "WORK_MEMORY_NUM_SAMPLES", "ENC_MODULE",
                                  "DEC_MODULE", "FUTURE_SECONDS", "FUTURE_NUM_SAMPLES", "ANTICIPATION_SECONDS", "ANTICIPATION_NUM_SAMPLES")}
        return {"INPUT": {"MODALITY": d["MODALITY"], "VISUAL_SIZE": d["VISUAL_SIZE"]},
                "DATA": {"DATA_NAME": d["DATA_NAME"], "NUM_CLASSES": d["NUM_CLASSES"]},
                "MODEL": {"FEATURE_HEAD": {"LINEAR_ENABLED": d["LINEAR_ENABLED"], "LINEAR_OUT_FEATURES": d["LINEAR_OUT_FEATURES"]}, "LSTR": lstr}}

    @classmethod
    def from_reference_dict(cls, cfg: Any) -> "OADConfig":
        """``cfg``: the reference's config as nested dicts or attribute nodes (a yacs ``CfgNode`` works without importing yacs).  The
        feature width comes from ``INPUT.VISUAL_SIZE`` or from ``INPUT.VISUAL_FEATURE`` through the reference's FEATURE_SIZES names."""
        size = _get(cfg, "INPUT.VISUAL_SIZE")
        if size is None:
            name = _get(cfg, "INPUT.VISUAL_FEATURE")
            if name not in FEATURE_SIZES:
                raise ValueError(f"INPUT.VISUAL_FEATURE = {name!r}: unknown feature; set INPUT.VISUAL_SIZE")
            size = FEATURE_SIZES[name]
        base = cls.__dataclass_fields__
        kw = dict(VISUAL_SIZE=int(size), MODALITY=_get(cfg, "INPUT.MODALITY", "visual"), DATA_NAME=_get(cfg, "DATA.DATA_NAME", "THUMOS"),
                  NUM_CLASSES=int(_get(cfg, "DATA.NUM_CLASSES", 22)), LINEAR_ENABLED=bool(_get(cfg, "MODEL.FEATURE_HEAD.LINEAR_ENABLED", True)),
                  LINEAR_OUT_FEATURES=int(_get(cfg, "MODEL.FEATURE_HEAD.LINEAR_OUT_FEATURES", 1024)))
        for k in ("NUM_HEADS", "DIM_FEEDFORWARD", "ACTIVATION", "LONG_MEMORY_NUM_SAMPLES", "WORK_MEMORY_NUM_SAMPLES", "ENC_MODULE", "DEC_MODULE",
                  "FUTURE_SECONDS", "FUTURE_NUM_SAMPLES", "ANTICIPATION_SECONDS", "ANTICIPATION_NUM_SAMPLES"):
            v = _get(cfg, "MODEL.LSTR." + k)
            if v is not None:
                kw[k] = v if not isinstance(base[k].default, int) else int(v)
        return cls(**kw)


# ------------------------------------------------------------------------------------------------ the parameter tree
class _Attention(nn.Module):
    def __init__(self, d: int):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d, d))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d))
        self.out_proj = nn.Linear(d, d)
        nn.init.xavier_uniform_(self.in_proj_weight)


class _Layer(nn.Module):
    def __init__(self, d: int, ffn: int, decoder: bool):
        super().__init__()
        self.self_attn = _Attention(d)
        if decoder:
            self.multihead_attn = _Attention(d)
        self.linear1 = nn.Linear(d, ffn)
        self.linear2 = nn.Linear(ffn, d)
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)
        if decoder:
            self.norm3 = nn.LayerNorm(d)


class _Stack(nn.Module):
    def __init__(self, d: int, ffn: int, decoder: bool, layers: int, norm: bool):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(d, ffn, decoder) for _ in range(layers)])
        if norm:
            self.norm = nn.LayerNorm(d)


class _FeatureHead(nn.Module):
    def __init__(self, d_in: int, d: int, linear: bool):
        super().__init__()
        self.visual_linear = nn.Sequential(nn.Linear(d_in, d), nn.LayerNorm(d), nn.ReLU(inplace=True)) if linear else nn.Identity()


class _PositionalEncoding(nn.Module):
    def __init__(self, d: int, max_len: int = PE_MAX_LEN):
        super().__init__()
        pe = torch.zeros(max_len, d)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d, 2).float() * (-math.log(10000.0) / d))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(0).transpose(0, 1))      # [max_len, 1, d], as the reference registers it


class DetectorState:
    """Device-resident state of ``streams`` independent streams of one detector (ring of projected long samples + cached compressed
    memory per stream)."""

    def __init__(self, detector: "OnlineActionDetector", streams: int):
        self.detector, self.streams = detector, int(streams)
        det_h = detector._handle_ptr()      # packs the weights if they have changed: the token below is the packed one
        self._token = detector._native.token
        self._h = nat.OwnedHandle(nat.lib.sf_oad_state_destroy, "DetectorState")
        with torch.cuda.device(detector.device):
            nat.check(nat.lib.sf_oad_state_create(det_h, self.streams, C.byref(self._h)))

    def fill(self, stream: int) -> int:
        n = nat.lib.sf_oad_state_fill(self._h, int(stream))
        if n < 0:
            nat.check(n)
        return n

    def reset(self, stream: Optional[int] = None) -> None:
        nat.check(nat.lib.sf_oad_state_reset(self._h, -1 if stream is None else int(stream)))

    def clone(self) -> "DetectorState":
        other = DetectorState(self.detector, self.streams)
        dev = self.detector.device
        for i in range(self.streams):
            nat.launch(dev, nat.lib.sf_oad_state_copy, other._h, i, self._h, i)
        return other


class OnlineActionDetector(nn.Module):
    def __init__(self, config: Any, compute_dtype: Any = "fp32", device: Any = None):
        super().__init__()
        if not isinstance(config, OADConfig):
            config = OADConfig.from_reference_dict(config)
        self._compute = nat.compute_mode(compute_dtype)
        self.config = config
        c = config
        d = self.d_model = c.d_model
        self.long_memory_num_samples, self.work_memory_num_samples = c.LONG_MEMORY_NUM_SAMPLES, c.WORK_MEMORY_NUM_SAMPLES
        self.num_classes = c.NUM_CLASSES
        nat.lib.sf_oad_destroy(self._create(0))      # the library's width rules, checked before any weight exists
        self.feature_head_long = _FeatureHead(c.VISUAL_SIZE, d, c.LINEAR_ENABLED)
        self.feature_head_work = _FeatureHead(c.VISUAL_SIZE, d, c.LINEAR_ENABLED)
        self.pos_encoding = _PositionalEncoding(d)
        self.enc_queries = nn.ModuleList([nn.Embedding(m[0], d) if m[0] != -1 else None for m in c.ENC_MODULE])
        self.enc_modules = nn.ModuleList([_Stack(d, c.DIM_FEEDFORWARD, m[0] != -1, m[1], bool(m[2])) for m in c.ENC_MODULE])
        self.dec_modules = _Stack(d, c.DIM_FEEDFORWARD, True, c.DEC_MODULE[1], bool(c.DEC_MODULE[2]))
        self.classifier = nn.Linear(d, c.NUM_CLASSES)
        self.ignored_keys: List[str] = []
        self._native = nat.PackedHandle(self._create, nat.lib.sf_oad_load_tensor, self._finalize, nat.lib.sf_oad_destroy, "detector")
        self._tensors = None                # the parameter / buffer objects, listed once: the per-step token reads their versions only
        self.requires_grad_(False)
        self.eval()
        if device is not None:
            self.to(device)

    # ------------------------------------------------------------------------------------ native handle
    def _create(self, device_index: int):
        c = self.config
        cfg = nat.SfOadConfig()
        cfg.d_in, cfg.d_model, cfg.heads, cfg.ffn = c.VISUAL_SIZE, c.d_model, c.NUM_HEADS, c.DIM_FEEDFORWARD
        cfg.long_samples, cfg.work_samples, cfg.classes = c.LONG_MEMORY_NUM_SAMPLES, c.WORK_MEMORY_NUM_SAMPLES, c.NUM_CLASSES
        cfg.act, cfg.linear_enabled, cfg.enc_modules = _ACT[c.ACTIVATION], int(bool(c.LINEAR_ENABLED)), len(c.ENC_MODULE)
        for j, m in enumerate(c.ENC_MODULE):
            cfg.enc_queries[j], cfg.enc_layers[j], cfg.enc_norm[j] = int(m[0]), int(m[1]), int(bool(m[2]))
        cfg.dec_layers, cfg.dec_norm, cfg.eps = int(c.DEC_MODULE[1]), int(bool(c.DEC_MODULE[2])), 1e-5
        h = C.c_void_p()
        code = nat.lib.sf_oad_create(C.byref(cfg), device_index, C.byref(h))
        if code == nat.SF_ERR_INVALID:
            raise ValueError((nat.lib.sf_last_error() or b"").decode(errors="replace"))
        nat.check(code)
        return h

    @property
    def device(self) -> torch.device:
        return self.classifier.weight.device

    def _finalize(self, h) -> None:
        nat.check(nat.lib.sf_oad_finalize(h, self._compute))

    def _items(self):
        rows = self.long_memory_num_samples + self.work_memory_num_samples
        return [(k, t[:rows, 0] if k == "pos_encoding.pe" else t) for k, t in self.state_dict().items()]

    def _handle_ptr(self):
        """The native detector, (re)packed when a parameter changed (in-place update, load_state_dict, .to(device)).  States made before
        a repack belong to the old weights and are refused."""
        dev = self.device
        if self._tensors is None:
            self._tensors = list(self.parameters()) + list(self.buffers())
        return self._native.get(dev, nat.weights_token(dev, self._tensors), self._items)

    # ------------------------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """A reference checkpoint's ``model_state_dict``.  The tensors of what the native detector does not compute (``gen_*``,
        ``final_query``, ``*_fusions``) are accepted, ignored and listed in ``ignored_keys``."""
        if "model_state_dict" in state_dict and not torch.is_tensor(state_dict["model_state_dict"]):
            state_dict = state_dict["model_state_dict"]
        sd, ignored = {}, []
        for k, v in state_dict.items():
            k2 = k[len("module."):] if k.startswith("module.") else k
            if k2.startswith(_IGNORED_PREFIXES):
                ignored.append(k2)
            else:
                sd[k2] = v
        self.ignored_keys = sorted(ignored)
        self._tensors = None                # assign=True replaces the parameter objects
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def _apply(self, fn, *args, **kwargs):
        self._tensors = None                # .to() / .float() may replace the parameter objects
        return super()._apply(fn, *args, **kwargs)

    # ------------------------------------------------------------------------------------ inference
    def forward(self, *args, **kwargs):
        field_ = self.config.generation_enabled
        if field_ is not None:
            raise NotImplementedError(f"MODEL.LSTR.{field_} > 0: future generation / anticipation (CCI) is not part of the native detector")
        raise NotImplementedError("the batch forward (top-k 'knn' attention) is not part of the native detector: use step(), the "
                                  "stream_inference path")

    def new_state(self, streams: int = 1) -> DetectorState:
        return DetectorState(self, streams)

    def _workspace(self, h, n: int) -> torch.Tensor:
        return self._native.workspace(nat.sized(nat.lib.sf_oad_workspace_bytes, h, n), self.device)

    @torch.no_grad()
    def step(self, work_features: torch.Tensor, long_features: Any = None, memory_key_padding_mask: Any = None, state: DetectorState = None,
             stream_ids: Optional[Sequence[int]] = None, probs: bool = False) -> torch.Tensor:
        """One step of ``n`` streams -> scores ``[n, W, C]`` (their softmax with ``probs=True``).

        ``work_features`` ``[n, W, d_in]`` (or ``[W, d_in]``).  ``long_features``: None, one tensor for every stream (``[n, 1 | L, d_in]``),
        or a list with one entry per stream, each None (reuse the cached compressed memory), ``[1, d_in]`` (one new sample; the oldest
        drops out) or ``[L, d_in]`` (the whole window, oldest first: the first step of an empty stream).  ``memory_key_padding_mask``:
        additive ``[n, L]`` (or ``[L]``) by window position, 0 = oldest, ``-inf`` allowed; it matters on steps that pass a long sample.
        Its values are checked on the host before launch: pass a CPU tensor (as ``padding_mask`` returns) on a latency-critical path, a
        device tensor costs a device-to-host copy and synchronisation here.
        """
        if self.config.generation_enabled is not None:
            raise NotImplementedError(f"MODEL.LSTR.{self.config.generation_enabled} > 0: future generation / anticipation (CCI) is not part of "
                                      "the native detector")
        L = self.long_memory_num_samples
        mask_cpu = None
        if memory_key_padding_mask is not None:      # checked before anything touches the device
            mask_cpu = torch.as_tensor(memory_key_padding_mask).detach().to("cpu", torch.float32)
            if mask_cpu.dim() == 1:
                mask_cpu = mask_cpu[None]
            if mask_cpu.dim() != 2 or mask_cpu.shape[1] != L or mask_cpu.shape[0] not in (1, work_features.shape[0] if work_features.dim() == 3 else 1):
                raise ValueError(f"memory_key_padding_mask must be [n, {L}] or [{L}], got {tuple(mask_cpu.shape)}")
            if bool(torch.isnan(mask_cpu).any()) or bool((mask_cpu == float("inf")).any()):
                raise ValueError("memory_key_padding_mask holds NaN or +inf")
            if bool((mask_cpu == float("-inf")).all(dim=1).any()):
                raise ValueError("memory_key_padding_mask masks every key of a stream (-inf everywhere): its queries would see nothing")
        if state is None:
            raise ValueError("step needs state=detector.new_state(streams=...)")
        h = self._handle_ptr()
        if state.detector is not self or state._token != self._native.token:
            raise ValueError("this state belongs to another detector (or to weights that have changed since): make a new_state()")
        dev = self.device
        L, W, d_in = self.long_memory_num_samples, self.work_memory_num_samples, self.config.VISUAL_SIZE
        work = work_features.to(device=dev, dtype=torch.float32)
        if work.dim() == 2:
            work = work[None]
        if work.dim() != 3 or work.shape[1:] != (W, d_in):
            raise ValueError(f"work_features must be [n, {W}, {d_in}], got {tuple(work_features.shape)}")
        n = work.shape[0]
        ids = list(range(n)) if stream_ids is None else [int(i) for i in stream_ids]
        if len(ids) != n or len(set(ids)) != n or any(i < 0 or i >= state.streams for i in ids):
            raise ValueError(f"stream_ids {ids}: {n} distinct streams of the state's {state.streams} expected")
        if n > nat.SF_OAD_MAX_CALL_STREAMS:
            raise ValueError(f"{n} streams in one call: at most {nat.SF_OAD_MAX_CALL_STREAMS}")
        if long_features is None:
            longs: List[Any] = [None] * n
        elif torch.is_tensor(long_features):
            lf = long_features[None] if long_features.dim() == 2 else long_features
            longs = list(lf)
        else:
            longs = list(long_features)
        if len(longs) != n:
            raise ValueError(f"long_features names {len(longs)} streams, work_features {n}")
        rows, counts = [], []
        for i, lg in enumerate(longs):
            if lg is None:
                counts.append(0)
                if state.fill(ids[i]) == 0:
                    raise ValueError(f"stream {ids[i]} is empty: its first step passes the whole long window [{L}, {d_in}]")
                continue
            lg = lg.to(device=dev, dtype=torch.float32).reshape(-1, lg.shape[-1])
            want = L if state.fill(ids[i]) == 0 else 1
            if lg.shape != (want, d_in):
                raise ValueError(f"stream {ids[i]}: long_features must be [{want}, {d_in}] here ({'empty stream: the whole window' if want == L else 'one new sample'}), "
                                 f"got {tuple(lg.shape)}")
            rows.append(lg)
            counts.append(want)
        mask = None
        if mask_cpu is not None and any(counts):
            mask = mask_cpu.expand(n, L).to(dev).contiguous()
        work = work.contiguous()
        long_dev = torch.cat(rows).contiguous() if rows else None
        out = torch.empty(n, W, self.num_classes, dtype=torch.float32, device=dev)
        nat.launch(dev, nat.lib.sf_oad_step, h, state._h, nat.i32_array(ids), n, work.data_ptr(), nat.ptr(long_dev), nat.i32_array(counts),
                   nat.ptr(mask), out.data_ptr(), int(bool(probs)), workspace=self._workspace(h, n))
        return out


def padding_mask(long_indices: Sequence[int]) -> torch.Tensor:
    """The reference's rule (``do_lstr_stream_inference``, lstr_inference.py:94-98) on the frame indices the long window holds, oldest
    first: with ``z`` leading entries equal to 0 (copies of frame 0: the initial fill, and frame 0 pushed again as a sample), the first
    ``z - 1`` slots are ``-inf``, so exactly one copy of frame 0 is visible.  A host tensor ``[L]``."""
    m = torch.zeros(len(long_indices), dtype=torch.float32)
    last_zero = bisect.bisect_right(list(long_indices), 0) - 1
    if last_zero > 0:
        m[:last_zero] = float("-inf")
    return m


class StreamingActionDetector:
    """One video stream through the streaming encoder and the detector: ``push(frame)`` -> the newest frame's class probabilities ``[C]``.

    Replaces the loop of the reference's ``do_lstr_stream_inference`` over saved features.  Frame ``t``'s feature is the encoder's
    ``pooler_output`` of the streamed frame (``pooling_method="last"``, as ``extract_oad_feature.py`` saves it).  The work window holds the
    last ``W`` features, padded with the first one while the stream is younger (the data layer's ``clip(0)``).  The long window starts as
    ``L`` copies of the first feature; frame ``j = t - W`` leaves the work window at push ``t`` and becomes a long sample when
    ``j % long_sample_rate == 0`` — frame 0 included, at ``t = W``, as in the reference's loop (``long_end % rate == 0`` with
    ``long_end = 0``).  ``long_indices`` records the frame index of every slot and the mask follows ``padding_mask(long_indices)``: the
    copies of frame 0 are masked but one, the pushed-again frame 0 counting as one more copy.
    """

    def __init__(self, tower: Any, detector: OnlineActionDetector, long_sample_rate: int = 4, max_frames: Optional[int] = None):
        if long_sample_rate < 1:
            raise ValueError("long_sample_rate must be >= 1")
        self.tower, self.detector, self.long_sample_rate = tower, detector, int(long_sample_rate)
        self._max_frames = max_frames
        self.reset()

    def reset(self) -> None:
        self.cache = None
        self.state = None
        self.features: deque = deque(maxlen=self.detector.work_memory_num_samples + 1)
        self.frames_seen = 0
        self.long_indices: List[int] = []
        self.last_features: Optional[torch.Tensor] = None

    @torch.no_grad()
    def push(self, frame: torch.Tensor) -> torch.Tensor:
        """``frame``: ``[C, H, W]`` (or ``[1, 1, C, H, W]``), what the tower's streaming forward takes."""
        det = self.detector
        L, W = det.long_memory_num_samples, det.work_memory_num_samples
        x = frame.reshape(1, 1, *frame.shape[-3:])
        if self.cache is None:
            self.cache = self.tower.new_cache(1, self._max_frames, x.shape[-2], x.shape[-1], policy="slide")
            self.state = det.new_state(1)
        out = self.tower(x.to(self.tower.device), past_key_values=self.cache)
        feat = out.pooler_output[:, -1].reshape(-1).float()
        self.last_features = feat
        self.features.append(feat)
        t = self.frames_seen
        self.frames_seen += 1
        long = mask = None
        if t == 0:
            long, self.long_indices = feat[None].expand(L, -1), [0] * L
        elif t - W >= 0 and (t - W) % self.long_sample_rate == 0:
            long = self.features[0][None]                                   # the frame that has just left the work window
            self.long_indices = self.long_indices[1:] + [t - W]
        if long is not None:
            mask = padding_mask(self.long_indices)[None]                    # on the host: step checks it without a synchronisation
        held = list(self.features)[-W:]
        work = torch.stack([held[0]] * (W - len(held)) + held)[None]
        return det.step(work, None if long is None else [long], mask, state=self.state, probs=True)[0, -1]
