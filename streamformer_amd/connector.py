"""The video-LLM connector on the HIP library: projector, spatial pooling and newline tokens.

Mirror of what the reference's VideoQA model does between its vision tower and its language model (``downstream/VideoQA/llava/model/
llava_arch.py``): ``mm_projector`` (``:213``, built by ``multimodal_projector/builder.py``), ``get_2dPool`` (``:171-190``) and the newline
placement (``:261-288``, ``:351-390``).  ``VideoTokenConnector`` carries the reference's parameter tree under the reference's key names
(``mm_projector.0.weight``, ``mm_projector.2.weight``, ..., ``image_newline``; a checkpoint's leading ``model.`` is accepted and dropped) and
reads the LLaVA config fields; the forward runs in ``libstreamformer_hip.so`` (``sf_connector_forward``, kernel in ``csrc/sf_connector.hip``).
Inference only: every parameter is born with ``requires_grad = False`` and the outputs carry no graph.

``StreamingVideoTokens`` joins a streaming ``TimesformerVisionTower`` to a connector: every push projects the NEW frames only and the
window's sequence is laid out again from the kept per-frame tokens (each frame's tokens depend on that frame's features alone).
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import re
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _native as nat
from .convert import read_state_dict

POOL_MODES = {"none": 0, "average": 1, "max": 2, "bilinear": 3}
NEWLINE_POSITIONS = {"no_token": 0, "one_token": 1, "frame": 2, "grid": 3}
_OUT_DTYPES = {torch.float32: nat.SF_F32, torch.bfloat16: nat.SF_BF16}


def _field(config: Any, name: str, default: Any = None) -> Any:
    if isinstance(config, dict):
        v = config.get(name, default)
    else:
        v = getattr(config, name, default)
    return default if v is None else v


def projector_depth(projector_type: str) -> int:
    """Linears of a ``mm_projector_type`` (``multimodal_projector/builder.py:32-65``): 0 identity, 1 linear, n for ``mlp{n}x_gelu``."""
    if projector_type == "linear":
        return 1
    if projector_type == "identity":
        return 0
    m = re.match(r"^mlp(\d+)x_gelu$", projector_type)
    if m and int(m.group(1)) >= 1:
        return int(m.group(1))
    if projector_type == "pooler" or re.match(r"^mlp(\d+)x_res(\d+)x_gelu$", projector_type):
        raise NotImplementedError(f"mm_projector_type {projector_type!r}: only 'linear', 'identity' and 'mlp<n>x_gelu' run natively")
    raise ValueError(f"Unknown projector type: {projector_type}")


def pooled_side(patches_per_side: int, mode: str, stride: int) -> int:
    """Cells per side after ``get_2dPool``: ceil(P / stride) for bilinear (``F.interpolate`` to a size), floor(P / stride) for the pools."""
    if stride <= 1 or mode == "none":
        return patches_per_side
    return -(-patches_per_side // stride) if mode == "bilinear" else patches_per_side // stride


class VideoTokenConnector(nn.Module):
    def __init__(self, config: Any, compute_dtype: Any = "fp32", out_dtype: torch.dtype = torch.float32, device: Any = None):
        super().__init__()
        self._compute = nat.compute_mode(compute_dtype)
        if out_dtype not in _OUT_DTYPES:
            raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
        if _field(config, "add_faster_video", False):
            raise NotImplementedError("add_faster_video=True: the slow-fast tokens are not part of the native connector")
        self.projector_type = str(_field(config, "mm_projector_type", "linear"))
        self.depth = projector_depth(self.projector_type)
        if _field(config, "mm_hidden_size") is None or _field(config, "hidden_size") is None:
            raise ValueError("the connector's config needs mm_hidden_size and hidden_size")
        self.in_dim, self.out_dim = int(_field(config, "mm_hidden_size")), int(_field(config, "hidden_size"))
        # prepare_inputs_labels_for_multimodal calls get_2dPool(image_feat), i.e. stride 2, when the recipe names none
        self.pool_stride = int(_field(config, "mm_spatial_pool_stride", 2))
        self.pool_mode = str(_field(config, "mm_spatial_pool_mode", "bilinear"))
        if self.pool_mode not in ("average", "max", "bilinear"):
            raise ValueError(f"Unexpected mm_spatial_pool_mode: {self.pool_mode}")
        if self.pool_stride < 1:
            raise ValueError(f"mm_spatial_pool_stride must be >= 1, got {self.pool_stride}")
        self.newline_position = str(_field(config, "mm_newline_position", "one_token"))
        if self.newline_position not in NEWLINE_POSITIONS:
            raise ValueError(f"Unexpected mm_newline_position: {self.newline_position}")
        self.patch_merge_type = str(_field(config, "mm_patch_merge_type", "flat"))
        if self.patch_merge_type != "flat" and not self.patch_merge_type.startswith("spatial"):
            raise ValueError(f"Unexpected mm_patch_merge_type: {self.patch_merge_type}")
        self.image_aspect_ratio = str(_field(config, "image_aspect_ratio", "square"))
        unpad = "unpad" in self.patch_merge_type
        # the rows the video branch adds (llava_arch:339-390): none on the flat path, and one_token only with "unpad" (:381-385)
        if self.patch_merge_type == "flat" or (self.newline_position == "one_token" and not unpad):
            self.newline = "no_token"
        else:
            self.newline = self.newline_position
        self.config = dict(mm_projector_type=self.projector_type, mm_hidden_size=self.in_dim, hidden_size=self.out_dim,
                           mm_spatial_pool_stride=self.pool_stride, mm_spatial_pool_mode=self.pool_mode,
                           mm_newline_position=self.newline_position, mm_patch_merge_type=self.patch_merge_type,
                           image_aspect_ratio=self.image_aspect_ratio)
        self.out_dtype = out_dtype
        self._probes: Dict[Tuple[int, int, int], nat.OwnedHandle] = {}
        # the library's width rules, checked here so that a refusal names the field before any weight exists; the handles stay for num_tokens
        self._probe(self._video_key())
        self._probe((0, 1, self._video_key()[2]))       # rows of `layout`: the same newline rule, no pool
        if self.depth == 0:
            self.mm_projector = nn.Identity()
        elif self.depth == 1:
            self.mm_projector = nn.Linear(self.in_dim, self.out_dim)
        else:
            mods: List[nn.Module] = [nn.Linear(self.in_dim, self.out_dim)]
            for _ in range(1, self.depth):
                mods += [nn.GELU(), nn.Linear(self.out_dim, self.out_dim)]
            self.mm_projector = nn.Sequential(*mods)
        if unpad or self.newline != "no_token":          # llava_arch:45-46, :107-109
            self.image_newline = nn.Parameter(torch.randn(self.out_dim) / math.sqrt(self.out_dim))
        # handles by (pool_mode, stride, newline) layout under one token; one workspace, the largest any call has needed since the pack
        self._native = nat.PackedHandle(self._create, nat.lib.sf_connector_load_tensor, self._finalize, nat.lib.sf_connector_destroy, "connector")
        self.requires_grad_(False)
        self.eval()
        if device is not None:
            self.to(device)

    # ------------------------------------------------------------------------------------ native handles
    def _video_key(self) -> Tuple[int, int, int]:
        return (POOL_MODES[self.pool_mode], self.pool_stride, NEWLINE_POSITIONS[self.newline])

    def _frames_key(self) -> Tuple[int, int, int]:
        return (POOL_MODES[self.pool_mode], self.pool_stride, 0)

    def _create(self, device_index: int, key: Tuple[int, int, int], h: Any = None):
        h = C.c_void_p() if h is None else h
        cfg = nat.SfConnectorConfig(self.in_dim, self.out_dim, self.depth, key[0], key[1], key[2])
        nat.check(nat.lib.sf_connector_create(C.byref(cfg), device_index, C.byref(h)))
        return h

    def _finalize(self, h) -> None:
        nat.check(nat.lib.sf_connector_finalize(h, self._compute))

    def _probe(self, key: Tuple[int, int, int]):
        """A handle without weights that answers ``sf_connector_num_tokens`` for one layout; a copied connector makes its own."""
        h = self._probes.get(key)
        if h is None:
            h = self._probes[key] = self._create(0, key, nat.OwnedHandle(nat.lib.sf_connector_destroy, "connector probe"))
        return h

    @property
    def device(self) -> torch.device:
        for p in self.parameters():
            return p.device
        return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")

    def __getstate__(self):
        return dict(self.__dict__, _probes={})

    def _handle(self, key: Tuple[int, int, int]):
        """The native connector of one (pool_mode, stride, newline) layout, (re)packed when a parameter changed (in-place update,
        load_state_dict, .to(device))."""
        params = list(self.named_parameters())
        dev = self.device
        return self._native.get(dev, nat.weights_token(dev, [p for _, p in params]),
                                lambda: [(k, p) for k, p in params if not (k == "image_newline" and key[2] == 0)], key)

    def _workspace(self, h, F: int, P: int) -> torch.Tensor:
        return self._native.workspace(nat.sized(nat.lib.sf_connector_workspace_bytes, h, F, P), self.device)

    def _run(self, key: Tuple[int, int, int], feats: torch.Tensor, P: int, out_dtype: torch.dtype) -> torch.Tensor:
        h = self._handle(key)
        dev = self.device
        F = feats.shape[0]
        x = feats.to(device=dev, dtype=torch.float32).contiguous()
        rows = C.c_int64()
        nat.check(nat.lib.sf_connector_num_tokens(h, F, P, C.byref(rows)))
        out = torch.empty(rows.value, self.out_dim, dtype=out_dtype, device=dev)
        ws = self._workspace(h, F, P)
        nat.launch(dev, nat.lib.sf_connector_forward, h, x.data_ptr(), F, P, out.data_ptr(), _OUT_DTYPES[out_dtype], workspace=ws)
        return out

    # ------------------------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Keys with or without LLaVA's leading ``model.``; with ``strict=False`` entries that are neither projector nor newline (the rest
        of a whole checkpoint) are ignored."""
        sd = {}
        for k, v in state_dict.items():
            k2 = k[len("model."):] if k.startswith("model.") else k
            if strict or k2.startswith("mm_projector.") or k2 == "image_newline":
                sd[k2] = v
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def save_pretrained(self, save_directory: str) -> None:
        """``config.json`` (the LLaVA fields) + ``mm_projector.bin`` with LLaVA's ``model.``-prefixed keys."""
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(self.config, f, indent=2, sort_keys=True)
        sd = {"model." + k: v.detach().to("cpu").contiguous() for k, v in self.state_dict().items()}
        torch.save(sd, os.path.join(save_directory, "mm_projector.bin"))

    @classmethod
    def from_pretrained(cls, directory: str, compute_dtype: Any = "fp32", out_dtype: torch.dtype = torch.float32, device: Any = None,
                        config: Any = None) -> "VideoTokenConnector":
        """``directory``: ``config.json`` + ``mm_projector.bin`` (LLaVA's adapter file) or ``mm_projector.safetensors`` / ``model.safetensors``
        (a whole checkpoint: the connector's entries are picked out)."""
        path = str(directory)
        if not os.path.isdir(path):
            raise OSError(f"{path!r} is not a local directory: pass the directory that holds config.json and mm_projector.bin")
        if config is None:
            with open(os.path.join(path, "config.json")) as f:
                config = json.load(f)
        sd = read_state_dict(path, ("mm_projector.bin", "mm_projector.safetensors", "model.safetensors"))
        model = cls(config, compute_dtype=compute_dtype, out_dtype=out_dtype)
        missing = model.load_state_dict(sd, strict=False).missing_keys
        if missing:
            raise RuntimeError(f"the checkpoint under {path!r} lacks {missing}")
        if device is None and torch.cuda.is_available():
            device = "cuda"
        if device is not None:
            model.to(device)
        return model

    # ------------------------------------------------------------------------------------ forward
    def num_tokens(self, frames: int, patches_per_side: int) -> int:
        """Rows of ``forward`` for a clip of ``frames`` frames of ``patches_per_side``^2 patches (``sf_connector_num_tokens``)."""
        n = C.c_int64()
        nat.check(nat.lib.sf_connector_num_tokens(self._probe(self._video_key()), int(frames), int(patches_per_side), C.byref(n)))
        return int(n.value)

    @staticmethod
    def _side(n_tokens: int) -> int:
        P = math.isqrt(n_tokens)
        if P < 1 or P * P != n_tokens:
            raise ValueError(f"{n_tokens} patch tokens per frame do not form a square grid")
        return P

    @torch.no_grad()
    def forward(self, features: torch.Tensor, modality: str = "video"):
        """``features`` (F, N, D) -> (tokens, D_llm); (B, T, N, D) -> one such tensor per clip.  ``modality="image"``: the projector
        alone (no pooling, no newline rows: the reference's flat path)."""
        if modality not in ("video", "image"):
            raise ValueError(f"Unexpected modality: {modality}")
        if modality == "image" and "anyres" in self.image_aspect_ratio:
            raise NotImplementedError(f"image_aspect_ratio {self.image_aspect_ratio!r}: the anyres image branches are not part of the native connector")
        if features.dim() == 4:
            return [self.forward(clip, modality) for clip in features]
        if features.dim() != 3 or features.shape[-1] != self.in_dim or features.shape[0] < 1:
            raise ValueError(f"features must be (F, N, {self.in_dim}) or (B, T, N, {self.in_dim}), got {tuple(features.shape)}")
        P = self._side(features.shape[1])
        key = self._video_key() if modality == "video" else (0, 1, 0)
        return self._run(key, features, P, self.out_dtype)

    @torch.no_grad()
    def project_frames(self, features: torch.Tensor) -> torch.Tensor:
        """(F, N, D) -> fp32 (F, P'^2, D_llm): the projected and pooled tokens of every frame, without newline rows."""
        P = self._side(features.shape[1])
        out = self._run(self._frames_key(), features, P, torch.float32)
        return out.reshape(features.shape[0], -1, self.out_dim)

    @torch.no_grad()
    def layout(self, frame_tokens: torch.Tensor) -> torch.Tensor:
        """fp32 (F, P'^2, D_llm) of ``project_frames`` -> the sequence of ``forward`` for those frames: rows placed and the newline rows
        written by the connector's layout kernel (identity taps)."""
        dev = self.device
        F, cells, D = frame_tokens.shape
        Po = self._side(cells)
        nl = NEWLINE_POSITIONS[self.newline]
        rows = C.c_int64()
        nat.check(nat.lib.sf_connector_num_tokens(self._probe((0, 1, nl)), F, Po, C.byref(rows)))
        x = frame_tokens.to(device=dev, dtype=torch.float32).contiguous()
        newline = self.image_newline.detach().to(device=dev, dtype=torch.float32).contiguous() if nl else None
        out = torch.empty(rows.value, D, dtype=self.out_dtype, device=dev)
        nat.launch(dev, nat.lib.sf_op_connector_pool, x.data_ptr(), None, None, F, Po, D, 0, 1, nl, nat.ptr(newline), out.data_ptr(),
                   _OUT_DTYPES[self.out_dtype], None, None)
        return out


class StreamingVideoTokens:
    """A streaming ``TimesformerVisionTower`` and a ``VideoTokenConnector``: ``push`` encodes and projects the new frames only, keeps the
    last ``context_length`` frames' tokens and returns the window's sequence — what the reference computes by projecting the whole
    returned window again on every call (vqa_enc:1532-1544 + llava_arch:198-213)."""

    def __init__(self, tower, connector: VideoTokenConnector):
        if not getattr(tower, "streaming_mode", False):
            raise ValueError("StreamingVideoTokens needs a vision tower in streaming_mode")
        if tower.hidden_size != connector.in_dim:
            raise ValueError(f"the tower's hidden_size {tower.hidden_size} is not the connector's mm_hidden_size {connector.in_dim}")
        self.tower = tower
        self.connector = connector
        self.context_length = int(tower.context_length)
        self._buf: Optional[torch.Tensor] = None        # [2 * context_length, P'^2, D_llm]: the window is the slice [start, start + held)
        self._start = 0
        self._held = 0

    def clear(self) -> None:
        self._start = self._held = 0
        self.tower.clear_cache()

    @property
    def frames_held(self) -> int:
        return self._held

    @torch.no_grad()
    def push(self, images: torch.Tensor) -> torch.Tensor:
        """``images``: the new frames of the stream, (1, T, C, H, W) -> the window's (tokens, D_llm)."""
        self.tower(images)
        new = self.tower.new_frame_features
        if new.shape[0] != 1:
            raise ValueError(f"StreamingVideoTokens follows one stream, got a batch of {new.shape[0]}")
        tok = self.connector.project_frames(new[0])[-self.context_length:]
        cap = 2 * self.context_length
        if self._buf is None or self._buf.shape[1:] != tok.shape[1:] or self._buf.device != tok.device:
            self._buf = torch.empty(cap, *tok.shape[1:], dtype=torch.float32, device=tok.device)
            self._start = self._held = 0
        T = tok.shape[0]
        keep = min(self._held, self.context_length - T)
        first = self._start + self._held - keep
        if first + keep + T > cap:                      # once per context_length pushes: the kept frames move to the front
            self._buf[:keep] = self._buf[first:first + keep].clone()
            first = 0
        self._buf[first + keep:first + keep + T] = tok
        self._start, self._held = first, keep + T
        return self.connector.layout(self._buf[self._start:self._start + self._held])
