"""The SigLIP text tower on the HIP library: captions and class prompts from token ids.

Mirror of HF ``SiglipTextModel`` as the reference's multitask wrapper holds it (``models/modeling_timesformer_siglip.py:1365-1375``,
frozen) and as every task head calls it: ``self.text_encoder(ids)[1]`` / ``self.text_encoder(**tokenizer_output)[1]``
(``:1680, 1756, 1997, 2104, 2217, 2315, 2385``).  The module carries HF's parameter tree under HF's key names
(``embeddings.token_embedding.weight``, ``encoder.layers.<i>.self_attn.q_proj.weight``, ..., ``final_layer_norm.*``, ``head.*``; a
checkpoint's leading ``text_model.`` is accepted and dropped), the forward runs in ``libstreamformer_hip.so`` (``sf_text_forward``,
kernels in ``csrc/sf_text.hip``).  Inference only: the tower is frozen in the reference, every parameter is born with
``requires_grad = False`` and the outputs carry no graph.

The tokenizer stays the caller's object: any callable ``tokenizer(list_of_str, padding="max_length", max_length=64, truncation=True,
return_tensors="pt")`` returning ``input_ids`` (and optionally ``attention_mask``) serves.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Any, Dict, Optional, Sequence

import torch
from torch import nn

from . import _native as nat
from .convert import read_state_dict, write_state_dict

_ACT_CODES = {"gelu": 0, "gelu_new": 1, "gelu_pytorch_tanh": 1, "relu": 2}
MAX_CAPTION_TOKENS = 64                   # the reference tokenises every caption and prompt to max_length = 64


class SiglipTextConfig:
    """The fields of HF ``SiglipTextConfig`` the tower reads, with HF's defaults (SigLIP-base)."""

    def __init__(self, vocab_size=32000, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                 max_position_embeddings=64, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6, projection_size=None, **unused):
        self.vocab_size = int(vocab_size)
        self.hidden_size = int(hidden_size)
        self.intermediate_size = int(intermediate_size)
        self.num_hidden_layers = int(num_hidden_layers)
        self.num_attention_heads = int(num_attention_heads)
        self.max_position_embeddings = int(max_position_embeddings)
        self.hidden_act = hidden_act
        self.layer_norm_eps = float(layer_norm_eps)
        self.projection_size = int(projection_size) if projection_size is not None else self.hidden_size

    def to_dict(self) -> Dict[str, Any]:
        return dict(vars(self), model_type="siglip_text_model")

    @classmethod
    def from_pretrained(cls, directory: str) -> "SiglipTextConfig":
        """``config.json`` of a text checkpoint (flat) or of a whole SigLIP model (fields under ``text_config``)."""
        with open(os.path.join(directory, "config.json")) as f:
            d = json.load(f)
        return cls(**d.get("text_config", d))


class TextModelOutput:
    """``[0]`` / ``.last_hidden_state`` [B, L, D], ``[1]`` / ``.pooler_output`` [B, projection] (HF's BaseModelOutputWithPooling)."""

    def __init__(self, last_hidden_state: torch.Tensor, pooler_output: torch.Tensor):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = pooler_output

    def to_tuple(self):
        return (self.last_hidden_state, self.pooler_output)

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return self.to_tuple()[i]

    def __iter__(self):
        return iter(self.to_tuple())

    def __len__(self):
        return 2


class _Embeddings(nn.Module):
    def __init__(self, c: SiglipTextConfig):
        super().__init__()
        self.token_embedding = nn.Embedding(c.vocab_size, c.hidden_size)
        self.position_embedding = nn.Embedding(c.max_position_embeddings, c.hidden_size)
        self.register_buffer("position_ids", torch.arange(c.max_position_embeddings).expand((1, -1)), persistent=False)


class _Attention(nn.Module):
    def __init__(self, D: int):
        super().__init__()
        self.k_proj = nn.Linear(D, D)
        self.v_proj = nn.Linear(D, D)
        self.q_proj = nn.Linear(D, D)
        self.out_proj = nn.Linear(D, D)


class _Mlp(nn.Module):
    def __init__(self, D: int, I: int):
        super().__init__()
        self.fc1 = nn.Linear(D, I)
        self.fc2 = nn.Linear(I, D)


class _Layer(nn.Module):
    def __init__(self, c: SiglipTextConfig):
        super().__init__()
        self.layer_norm1 = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.self_attn = _Attention(c.hidden_size)
        self.layer_norm2 = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.mlp = _Mlp(c.hidden_size, c.intermediate_size)


class _Encoder(nn.Module):
    def __init__(self, c: SiglipTextConfig):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(c) for _ in range(c.num_hidden_layers)])


def pack_qkv(state_dict: Dict[str, torch.Tensor], layer: int):
    """The packed ``[3D, D]`` weight and ``[3D]`` bias of one layer's q / k / v projections, in the order the library packs them."""
    p = f"encoder.layers.{layer}.self_attn."
    return (torch.cat([state_dict[p + f"{n}_proj.weight"] for n in "qkv"], dim=0),
            torch.cat([state_dict[p + f"{n}_proj.bias"] for n in "qkv"], dim=0))


def normalize_text_keys(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Text-tower entries of a checkpoint under this module's key names: a leading ``text_model.`` dropped, vision-tower and scalar
    entries of a whole ``SiglipModel`` checkpoint left out."""
    out = {}
    for k, v in state_dict.items():
        if k.startswith("vision_model.") or k in ("logit_scale", "logit_bias"):
            continue
        k = k[len("text_model."):] if k.startswith("text_model.") else k
        if k.endswith("position_ids"):
            continue
        out[k] = v
    return out


class SiglipTextModel(nn.Module):
    config_class = SiglipTextConfig
    main_input_name = "input_ids"

    def __init__(self, config: SiglipTextConfig, compute_dtype: Any = "fp32", device: Any = None):
        super().__init__()
        c = config
        if c.hidden_act not in _ACT_CODES:
            raise ValueError(f"unsupported hidden_act {c.hidden_act!r}")
        self._compute = nat.compute_mode(compute_dtype)
        self.config = c
        nat.lib.sf_text_destroy(self._create(0))      # the library's width rules, checked here so that a refusal names the field before any weight exists
        self.embeddings = _Embeddings(c)
        self.encoder = _Encoder(c)
        self.final_layer_norm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.head = nn.Linear(c.hidden_size, c.projection_size)
        self._native = nat.PackedHandle(self._create, nat.lib.sf_text_load_tensor, self._finalize, nat.lib.sf_text_destroy, "text tower",
                                        refusal="the text tower runs on the MI355X: move the model with .to('cuda') (there is no CPU fallback)")
        self.requires_grad_(False)
        self.eval()
        if device is not None:
            self.to(device)

    def _native_config(self) -> "nat.SfTextConfig":
        c = self.config
        return nat.SfTextConfig(c.vocab_size, c.max_position_embeddings, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                                c.intermediate_size, c.projection_size, _ACT_CODES[c.hidden_act], c.layer_norm_eps)

    def _create(self, device_index: int):
        h = C.c_void_p()
        nat.check(nat.lib.sf_text_create(C.byref(self._native_config()), device_index, C.byref(h)))
        return h

    def _finalize(self, h) -> None:
        nat.check(nat.lib.sf_text_finalize(h, self._compute))

    # ------------------------------------------------------------------------------------ weights
    @property
    def device(self) -> torch.device:
        return self.head.weight.device

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        return super().load_state_dict(normalize_text_keys(state_dict), strict=strict, assign=assign)

    @classmethod
    def from_pretrained(cls, directory: str, compute_dtype: Any = "fp32", device: Any = None, config: Optional[SiglipTextConfig] = None):
        """``directory``: ``config.json`` + ``model.safetensors`` / ``pytorch_model.bin`` of a ``SiglipTextModel`` or a whole
        ``SiglipModel`` (the text entries are picked out)."""
        path = str(directory)
        if not os.path.isdir(path):
            raise OSError(f"{path!r} is not a local directory: download the checkpoint (config.json + model.safetensors or "
                          "pytorch_model.bin) and pass its directory")
        cfg = config or SiglipTextConfig.from_pretrained(path)
        model = cls(cfg, compute_dtype=compute_dtype)
        model.load_state_dict(read_state_dict(path, ("model.safetensors", "pytorch_model.bin")), strict=True)
        if device is None and torch.cuda.is_available():
            device = "cuda"
        if device is not None:
            model.to(device)
        return model

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True) -> None:
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(self.config.to_dict(), f, indent=2, sort_keys=True)
        write_state_dict(save_directory, self.state_dict(), "model.safetensors" if safe_serialization else "pytorch_model.bin", safe_serialization)

    @property
    def _handle(self):
        return self._native.handles.get(None)

    def _packed(self):
        """The native tower, (re)packed when the parameters changed (in-place update, load_state_dict, .to(device))."""
        params = list(self.named_parameters())
        dev = self.device
        return self._native.get(dev, nat.weights_token(dev, [p for _, p in params]), params)

    def _workspace(self, h, B: int, L: int) -> torch.Tensor:
        ws = self._native.workspaces.get((B, L))
        if ws is None:
            n = nat.sized(nat.lib.sf_text_workspace_bytes, h, B, L)
            self._native.workspaces.clear()      # one shape at a time: class tables are large
            ws = self._native.workspace(n, self.device, (B, L))
        return ws

    # ------------------------------------------------------------------------------------ forward
    def _check_inputs(self, input_ids, attention_mask, position_ids):
        """Everything the kernels cannot refuse themselves, before anything is packed or launched."""
        c = self.config
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        ids = input_ids.reshape(-1, input_ids.shape[-1])
        B, L = ids.shape
        if B == 0 or L == 0:
            raise ValueError(f"input_ids must hold at least one token per caption, got shape {tuple(input_ids.shape)}")
        if L > c.max_position_embeddings:
            raise ValueError(f"sequence length {L} exceeds max_position_embeddings {c.max_position_embeddings}")
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= c.vocab_size:
            raise ValueError(f"input_ids outside the vocabulary [0, {c.vocab_size}): found {lo if lo < 0 else hi}")
        mask = None
        if attention_mask is not None:
            mask = attention_mask.reshape(-1, attention_mask.shape[-1]) != 0
            if tuple(mask.shape) != (B, L):
                raise ValueError(f"attention_mask must be [{B}, {L}], got {tuple(attention_mask.shape)}")
            empty = (~mask.any(dim=1)).nonzero().flatten().tolist()
            if empty:
                raise ValueError(f"attention_mask row {empty[0]} has no valid key: a caption needs at least one unmasked token")
        if position_ids is not None:
            want = torch.arange(L, device=position_ids.device).expand(position_ids.reshape(-1, position_ids.shape[-1]).shape[0], L)
            if position_ids.shape[-1] != L or not torch.equal(position_ids.reshape(-1, L).long(), want):
                raise NotImplementedError("position_ids other than arange(L): the embedding kernel adds position_embedding[l] to token l")
        return ids, mask

    def _device_inputs(self, ids, mask):
        dev = self.device
        ids_d = ids.to(dev, torch.int32).contiguous()
        mask_d = None if mask is None else mask.to(dev, torch.uint8).contiguous()
        return ids_d, mask_d

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, return_dict: bool = True, **unused):
        ids, mask = self._check_inputs(input_ids, attention_mask, position_ids)
        h = self._packed()
        c, dev = self.config, self.device
        B, L = ids.shape
        ids_d, mask_d = self._device_inputs(ids, mask)
        last = torch.empty(B, L, c.hidden_size, dtype=torch.float32, device=dev)
        pooled = torch.empty(B, c.projection_size, dtype=torch.float32, device=dev)
        nat.launch(dev, nat.lib.sf_text_forward, h, ids_d.data_ptr(), nat.ptr(mask_d), B, L, last.data_ptr(), pooled.data_ptr(),
                   workspace=self._workspace(h, B, L))
        last = last.reshape(*input_ids.shape, c.hidden_size)
        out = TextModelOutput(last, pooled)
        return out if return_dict else out.to_tuple()

    @torch.no_grad()
    def encode_groups(self, input_ids, group: int, attention_mask=None) -> torch.Tensor:
        """Class-prompt table rows: ``input_ids`` [labels * group, L], the prompts of one label consecutive -> [labels, projection]
        unit-norm rows (each pooled row normalised, the group averaged, the mean normalised; ``sf_text_forward_groups``)."""
        ids, mask = self._check_inputs(input_ids, attention_mask, None)
        B, L = ids.shape
        if group < 1 or B % group:
            raise ValueError(f"{B} prompts are not whole groups of {group}")
        h = self._packed()
        dev = self.device
        ids_d, mask_d = self._device_inputs(ids, mask)
        table = torch.empty(B // group, self.config.projection_size, dtype=torch.float32, device=dev)
        nat.launch(dev, nat.lib.sf_text_forward_groups, h, ids_d.data_ptr(), nat.ptr(mask_d), B, L, group, table.data_ptr(),
                   workspace=self._workspace(h, B, L))
        return table


def tokenize(text_tokenizer, texts: Sequence[str]) -> Dict[str, torch.Tensor]:
    """The tokenizer call of the reference's heads (modeling:2231-2233, 2308-2314): padded / truncated to 64 tokens, torch tensors."""
    enc = text_tokenizer(list(texts), return_tensors="pt", padding="max_length", max_length=MAX_CAPTION_TOKENS, truncation=True)
    return {k: enc[k] for k in ("input_ids", "attention_mask") if k in enc}


def encode_captions(text_encoder, text_tokenizer, captions: Sequence[str]) -> torch.Tensor:
    """``text_encoder(**text_tokenizer(captions, ...))[1]`` (modeling:2307-2316): [len(captions), projection], un-normalised."""
    enc = tokenize(text_tokenizer, captions)
    dev = text_encoder.device
    return text_encoder(**{k: v.to(dev) for k, v in enc.items()})[1]


PROMPTS_PER_CALL = 1024                   # class tables are encoded in chunks of whole labels: 1024 prompts of 64 tokens are 64 Ki rows


def encode_label_prompts(text_encoder, text_tokenizer, labels: Sequence[str], templates: Sequence[str]) -> torch.Tensor:
    """The prompt-ensemble class table of ``prepare_multi_task`` (modeling:2207-2223): every label is written into every template
    (``template.format(label)``), the prompts are tokenised to 64 tokens and encoded from their ids alone (no attention mask, as the
    reference calls the tower there), each pooled row is L2-normalised, the rows of a label are averaged and the mean is normalised:
    [len(labels), projection], unit-norm rows."""
    labels, templates = list(labels), list(templates)
    if not labels or not templates:
        raise ValueError("encode_label_prompts needs at least one label and one template")
    G = len(templates)
    per_call = max(1, PROMPTS_PER_CALL // G)
    rows = []
    for i in range(0, len(labels), per_call):
        texts = [t.format(label) for label in labels[i:i + per_call] for t in templates]
        ids = tokenize(text_tokenizer, texts)["input_ids"]
        if isinstance(text_encoder, SiglipTextModel):
            rows.append(text_encoder.encode_groups(ids.to(text_encoder.device), G))
        else:                              # another tower with the same call form (a test double): the same rule in torch
            out = text_encoder(ids.to(text_encoder.device))[1].float()
            out = out / out.norm(p=2, dim=-1, keepdim=True)
            out = out.reshape(-1, G, out.shape[-1]).mean(dim=1)
            rows.append(out / out.norm(p=2, dim=-1, keepdim=True))
    return torch.cat(rows, dim=0)
