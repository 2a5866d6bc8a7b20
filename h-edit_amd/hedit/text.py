"""Tokenizer / text-encoder stand-ins for offline runs.

The reference takes both from the SD pipeline (transformers CLIPTokenizer / CLIPTextModel,
text-guided/inversion/inversion_utils.py:25-33) and calls them twice per image -- they are not on
the accelerated path and no vocabulary / weights exist offline.  These classes
give the same call surface with synthetic weights; real transformers objects can be passed to
HEditPipeline instead.
"""
import math
import types

import torch
import torch.nn as nn

from .native import NativeOwner


class WordTokenizer:
    """Whitespace word-level tokenizer with the CLIPTokenizer surface used by the path
    (``__call__(...).input_ids``, ``encode``, ``decode``, ``model_max_length``)."""
    model_max_length = 77
    bos_token_id, eos_token_id = 49406, 49407

    def __init__(self, vocab_size=49408, stable_ids=False):
        self.vocab_size = vocab_size
        self.stable_ids = stable_ids
        self._ids = {}
        self._words = {}

    @staticmethod
    def _hash_id(w, attempt, n_ids):
        import hashlib
        key = w if attempt == 0 else f"{w}\x00{attempt}"
        return 1 + int.from_bytes(hashlib.sha256(key.encode("utf-8")).digest()[:8], "big") % n_ids

    def _id(self, w):
        # default: ids in order of first sight (what the committed golden vectors were generated with).  stable_ids: a
        # word's id is a function of the word ALONE (64 bits of SHA-256 into the id range), so a synthetic-weights run
        # gives a prompt the same embedding whether its image is edited alone or inside a lock-step batch (the drivers'
        # --random_init pipelines).  The id range has ~49 k slots, so a real prompt set (a few hundred distinct words)
        # does see collisions: the later word is then re-hashed with a counter until it finds a free id -- deterministic
        # for a given order of first sight, and reported once per word, because for THAT word the id now does depend
        # on what was tokenised before it.  `prescan` assigns the ids of a known vocabulary in sorted order up front,
        # which removes that dependence altogether (the drivers call it with every prompt of the run).
        if w not in self._ids:
            if len(self._ids) >= self.bos_token_id - 1:
                raise RuntimeError("WordTokenizer vocabulary exhausted")
            i = 1 + len(self._ids)
            if self.stable_ids:
                n_ids = self.bos_token_id - 1
                attempt = 0
                i = self._hash_id(w, 0, n_ids)
                while i in self._words:
                    attempt += 1
                    i = self._hash_id(w, attempt, n_ids)
                if attempt:
                    import warnings
                    warnings.warn(f"WordTokenizer(stable_ids): {w!r} collides with {self._words[self._hash_id(w, 0, n_ids)]!r}; "
                                  f"re-hashed to id {i} (attempt {attempt}) -- for this word the id depends on the order of "
                                  "first sight; call prescan() with the run's prompts to make it order-independent", stacklevel=3)
            self._ids[w] = i
            self._words[i] = w
        return self._ids[w]

    def prescan(self, prompts):
        """Assign the ids of every word of `prompts` now, in sorted word order: with stable_ids a collision is then
        resolved the same way whatever order the prompts are tokenised in later (batch invariance of a whole run)."""
        words = sorted({w for p in prompts for w in p.split(" ") if w != ""})
        for w in words:
            self._id(w)
        return len(words)

    def encode(self, text):
        return [self.bos_token_id] + [self._id(w) for w in text.split(" ") if w != ""] + [self.eos_token_id]

    def decode(self, ids):
        if isinstance(ids, int):          # one id, as CLIPTokenizer.decode accepts it (the attention viewers label maps so)
            ids = [ids]
        sp ={self.bos_token_id: "<|startoftext|>", self.eos_token_id: "<|endoftext|>"}
        return "".join(sp.get(int(i), self._words.get(int(i), "?")) for i in ids)

    def __call__(self, prompts, padding="max_length", max_length=None, truncation=True, return_tensors="pt"):
        if isinstance(prompts, str):
            prompts = [prompts]
        max_length = max_length or self.model_max_length
        rows = []
        for p in prompts:
            ids = self.encode(p)[:max_length]
            rows.append(ids + [self.eos_token_id] * (max_length - len(ids)))
        return types.SimpleNamespace(input_ids=torch.tensor(rows, dtype=torch.int64))


def prescan_prompts(tokenizer, records):
    """Give a stand-in tokenizer the whole vocabulary of a run before any work starts (a no-op for real tokenizers,
    which have no `prescan`).  `records`: dataset entries with ``original_prompt`` / ``editing_prompt`` as the drivers
    read them (the demo file calls them ``source_prompt`` / ``target_prompt``; square brackets around the edited words are stripped there, so they are stripped here).  Every rank
    of a sharded run passes the FULL dataset, so the ids do not depend on the shard either."""
    if not hasattr(tokenizer, "prescan"):
        return 0
    prompts = []
    for r in records:
        for k in ("original_prompt", "editing_prompt", "source_prompt", "target_prompt"):
            if isinstance(r, dict) and r.get(k):
                prompts.append(r[k].replace("[", "").replace("]", ""))
    return tokenizer.prescan(prompts)


class ClipTextEncoder(nn.Module):
    """CLIP-text-shaped transformer (pre-LN, causal, quick-GELU) with seeded random weights.
    forward(ids) -> (last_hidden_state,) like transformers' CLIPTextModel."""

    def __init__(self, dim=768, layers=12, heads=12, vocab=49408, max_len=77, seed=7):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.dim, self.heads = dim, heads
        self.tok = nn.Parameter(torch.randn(vocab, dim, generator=g) * 0.02)
        self.pos = nn.Parameter(torch.randn(max_len, dim, generator=g) * 0.01)
        blk = []
        for _ in range(layers):
            blk.append(nn.ParameterDict({
                "ln1_w": nn.Parameter(torch.ones(dim)), "ln1_b": nn.Parameter(torch.zeros(dim)),
                "qkv": nn.Parameter(torch.randn(3 * dim, dim, generator=g) / math.sqrt(dim)),
                "qkv_b": nn.Parameter(torch.zeros(3 * dim)),
                "out": nn.Parameter(torch.randn(dim, dim, generator=g) / math.sqrt(dim)),
                "out_b": nn.Parameter(torch.zeros(dim)),
                "ln2_w": nn.Parameter(torch.ones(dim)), "ln2_b": nn.Parameter(torch.zeros(dim)),
                "fc1": nn.Parameter(torch.randn(4 * dim, dim, generator=g) / math.sqrt(dim)),
                "fc1_b": nn.Parameter(torch.zeros(4 * dim)),
                "fc2": nn.Parameter(torch.randn(dim, 4 * dim, generator=g) / math.sqrt(4 * dim)),
                "fc2_b": nn.Parameter(torch.zeros(dim)),
            }))
        self.blocks = nn.ModuleList(blk)
        self.lnf_w = nn.Parameter(torch.ones(dim))
        self.lnf_b = nn.Parameter(torch.zeros(dim))
        for p in self.parameters():
            p.requires_grad_(False)

    def forward(self, ids):
        F = torch.nn.functional
        b, n = ids.shape
        h = self.tok[ids] + self.pos[:n][None]
        mask = torch.full((n, n), float("-inf"), device=h.device).triu(1)
        hd = self.dim // self.heads
        for p in self.blocks:
            x = F.layer_norm(h, (self.dim,), p["ln1_w"], p["ln1_b"])
            q, k, v = F.linear(x, p["qkv"], p["qkv_b"]).chunk(3, dim=-1)
            q, k, v = (t.reshape(b, n, self.heads, hd).transpose(1, 2) for t in (q, k, v))
            a = (q @ k.transpose(-1, -2)) * hd ** -0.5 + mask
            o = (a.softmax(-1) @ v).transpose(1, 2).reshape(b, n, self.dim)
            h = h + F.linear(o, p["out"], p["out_b"])
            x = F.layer_norm(h, (self.dim,), p["ln2_w"], p["ln2_b"])
            x = F.linear(x, p["fc1"], p["fc1_b"])
            h = h + F.linear(x * torch.sigmoid(1.702 * x), p["fc2"], p["fc2_b"])
        return (F.layer_norm(h, (self.dim,), self.lnf_w, self.lnf_b),)


# ---------------------------------------------------------------------------------------------- native prompt encoder
_BLOCK_SHAPES = (("ln_1.weight", (1,)), ("ln_1.bias", (1,)), ("attn.in_proj_weight", (3, 1)), ("attn.in_proj_bias", (3,)),
                 ("attn.out_proj.weight", (1, 1)), ("attn.out_proj.bias", (1,)), ("ln_2.weight", (1,)), ("ln_2.bias", (1,)),
                 ("mlp.c_fc.weight", (4, 1)), ("mlp.c_fc.bias", (4,)), ("mlp.c_proj.weight", (1, 4)), ("mlp.c_proj.bias", (1,)))
# transformers CLIPTextModel -> OpenAI CLIP, per layer (q / k / v are concatenated in that order into in_proj_*)
_HF_BLOCK = (("layer_norm1", "ln_1"), ("self_attn.out_proj", "attn.out_proj"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
             ("mlp.fc2", "mlp.c_proj"))
_STANDIN_BLOCK = (("ln1_w", "ln_1.weight"), ("ln1_b", "ln_1.bias"), ("qkv", "attn.in_proj_weight"), ("qkv_b", "attn.in_proj_bias"),
                  ("out", "attn.out_proj.weight"), ("out_b", "attn.out_proj.bias"), ("ln2_w", "ln_2.weight"), ("ln2_b", "ln_2.bias"),
                  ("fc1", "mlp.c_fc.weight"), ("fc1_b", "mlp.c_fc.bias"), ("fc2", "mlp.c_proj.weight"), ("fc2_b", "mlp.c_proj.bias"))
# entries of a full OpenAI CLIP state_dict that are not the text tower's (the TorchScript archive also stores three sizes)
_CLIP_NOT_TEXT = ("logit_scale", "input_resolution", "context_length", "vocab_size")


def text_param_shapes(width, layers, vocab_size, context_length, proj_dim=0):
    """The native executor's parameter table (csrc/text.hip: OpenAI CLIP state_dict names), name -> shape, in its order."""
    out = {"token_embedding.weight": (vocab_size, width), "positional_embedding": (context_length, width)}
    for i in range(layers):
        for name, mult in _BLOCK_SHAPES:
            out[f"transformer.resblocks.{i}.{name}"] = tuple(m * width for m in mult)
    out["ln_final.weight"] = (width,)
    out["ln_final.bias"] = (width,)
    if proj_dim:
        out["text_projection"] = (width, proj_dim)
    return out


def _cfg_get(config, key, default=None):
    return config.get(key, default) if isinstance(config, dict) else getattr(config, key, default)


def hf_to_clip_names(sd, layers):
    """transformers CLIPTextModel(WithProjection) names, with or without the ``text_model.`` prefix (transformers 5.x
    drops it), -> OpenAI CLIP names.  Keys this function does not know are passed through under their own name, so the
    strict check of the caller reports them as unexpected."""
    sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}
    sd.pop("embeddings.position_ids", None)              # an index buffer older checkpoints persist, not a parameter
    out, used = {}, set()

    def take(src, dst):
        if src in sd:
            out[dst] = sd[src]
            used.add(src)

    take("embeddings.token_embedding.weight", "token_embedding.weight")
    take("embeddings.position_embedding.weight", "positional_embedding")
    take("final_layer_norm.weight", "ln_final.weight")
    take("final_layer_norm.bias", "ln_final.bias")
    if "text_projection.weight" in sd:                   # nn.Linear [proj][width], no bias; CLIP multiplies by [width][proj]
        out["text_projection"] = sd["text_projection.weight"].t().contiguous()
        used.add("text_projection.weight")
    for i in range(layers):
        src, dst = f"encoder.layers.{i}.", f"transformer.resblocks.{i}."
        for a, b in _HF_BLOCK:
            for s in ("weight", "bias"):
                take(f"{src}{a}.{s}", f"{dst}{b}.{s}")
        for s in ("weight", "bias"):
            parts = [f"{src}self_attn.{p}_proj.{s}" for p in "qkv"]
            if all(p in sd for p in parts):
                out[f"{dst}attn.in_proj_{s}"] = torch.cat([sd[p] for p in parts], dim=0)
            used.update(p for p in parts if p in sd)     # a partial set surfaces as a missing in_proj_* entry
    for k, v in sd.items():
        if k not in used:
            out[k] = v
    return out


def standin_to_clip_names(enc):
    """The tensors of the torch stand-in ``ClipTextEncoder`` under the OpenAI CLIP names."""
    out = {"token_embedding.weight": enc.tok, "positional_embedding": enc.pos, "ln_final.weight": enc.lnf_w, "ln_final.bias": enc.lnf_b}
    for i, blk in enumerate(enc.blocks):
        for a, b in _STANDIN_BLOCK:
            out[f"transformer.resblocks.{i}.{b}"] = blk[a]
    return out


class TextEncoderOutput:
    """Indexes like transformers' BaseModelOutputWithPooling: [0] last_hidden_state (B, L, width), [1] pooler_output."""

    def __init__(self, last_hidden_state, pooler_output):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = pooler_output

    def __getitem__(self, i):
        return (self.last_hidden_state, self.pooler_output)[i]

    def __iter__(self):
        return iter((self.last_hidden_state, self.pooler_output))

    def __len__(self):
        return 2


class NativeClipText(NativeOwner):
    """The CLIP text transformer on the native executor (``hedit_text_*`` of libhedit_hip.so, csrc/text.hip): a parameter
    container under the OpenAI CLIP names plus the native handle.  There is no torch forward.  ``model.text_encoder(ids)[0]``
    works as with transformers' CLIPTextModel; results are bit-identical whatever the batch (``batch_invariant``), so
    ``HEditEngine.encode`` makes one call for all prompts.

    Pool position of ``[1]``: ``input_ids.argmax(-1)`` (the reference's rule, clip/model.py:378, and transformers' when the
    config carries the legacy ``eos_token_id = 2`` as SD-1.x checkpoints do) unless another ``eos_token_id`` is given,
    then the first occurrence of it (transformers' modeling_clip.py)."""
    batch_invariant = True
    _family = "text"

    def __init__(self, width, layers, heads, vocab_size, context_length, proj_dim=0, eos_token_id=None, device="cuda:0"):
        if width % heads or width // heads != 64:
            raise NotImplementedError(f"the native text encoder has head dimension 64, not {width}/{heads} (width/heads)")
        if proj_dim and proj_dim % 4:
            raise NotImplementedError(f"text_projection with {proj_dim} columns: the native text encoder needs a multiple of 4")
        self.width, self.layers, self.heads = int(width), int(layers), int(heads)
        self.vocab_size, self.context_length, self.proj_dim = int(vocab_size), int(context_length), int(proj_dim or 0)
        self.eos_token_id = None if eos_token_id in (None, 2) else int(eos_token_id)
        self.device = torch.device(device)
        self.param_shapes = text_param_shapes(self.width, self.layers, self.vocab_size, self.context_length, self.proj_dim)
        self.params = None
        self.calls = 0                # native encode calls made (tests count them)
        self._need = {}               # workspace bytes per (B, L): the query is a dry run of the whole forward

    # ------------------------------------------------------------------ parameters
    def load_state_dict(self, sd):
        """Strict: ``sd`` holds exactly the table's names (OpenAI CLIP), with the table's shapes."""
        missing = [k for k in self.param_shapes if k not in sd]
        extra = [k for k in sd if k not in self.param_shapes]
        if missing or extra:
            raise KeyError(f"state_dict mismatch: missing {missing[:5]} ({len(missing)}), unexpected {extra[:5]} ({len(extra)})")
        for k, shape in self.param_shapes.items():
            if tuple(sd[k].shape) != shape:
                raise ValueError(f"{k}: expected shape {shape}, got {tuple(sd[k].shape)}")
        self.params = {k: sd[k].detach() for k in self.param_shapes}
        self._native_release()
        return self

    def state_dict(self):
        return dict(self.params or {})

    @classmethod
    def from_clip_state_dict(cls, sd, device="cuda:0", eos_token_id=None):
        """A full OpenAI CLIP state_dict (``visual.*`` and the scalar entries are not the text tower's and are ignored)."""
        sd = {k: v for k, v in sd.items() if not k.startswith("visual.") and k not in _CLIP_NOT_TEXT}
        for k in ("token_embedding.weight", "positional_embedding"):
            if k not in sd:
                raise KeyError(f"state_dict mismatch: missing ['{k}'] (1), unexpected [] (0)")
        vocab, width = sd["token_embedding.weight"].shape
        layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
        proj = sd["text_projection"].shape[1] if "text_projection" in sd else 0
        if width % 64:
            raise NotImplementedError(f"the native text encoder has head dimension 64; width {width} is not a multiple of it")
        return cls(width, layers, width // 64, vocab, sd["positional_embedding"].shape[0], proj, eos_token_id, device).load_state_dict(sd)

    @staticmethod
    def check_hf_config(config):
        """(hidden_size, heads) of a transformers text config this executor implements, else NotImplementedError by name"""
        act = _cfg_get(config, "hidden_act", "quick_gelu")
        if act != "quick_gelu":
            raise NotImplementedError(f"hidden_act {act!r}: the native text encoder implements quick_gelu only")
        width, heads = int(_cfg_get(config, "hidden_size")), int(_cfg_get(config, "num_attention_heads"))
        if width % heads or width // heads != 64:
            raise NotImplementedError(f"head dimension {width / heads:g} (hidden_size {width} / num_attention_heads {heads}): "
                                      "the native text encoder implements 64 only")
        return width, heads

    @classmethod
    def from_hf_state_dict(cls, sd, config, device="cuda:0"):
        """transformers CLIPTextModel weights (either prefix) + its config (a dict, e.g. text_encoder/config.json, or a
        CLIPTextConfig).  SD-2.x's text model (gelu, other head sizes) is refused."""
        width, heads = cls.check_hf_config(config)
        layers = int(_cfg_get(config, "num_hidden_layers"))
        mapped = hf_to_clip_names(sd, layers)
        proj = mapped["text_projection"].shape[1] if "text_projection" in mapped else 0
        return cls(width, layers, heads, int(_cfg_get(config, "vocab_size")), int(_cfg_get(config, "max_position_embeddings")), proj,
                   _cfg_get(config, "eos_token_id"), device).load_state_dict(mapped)

    @classmethod
    def from_standin(cls, enc, device=None):
        """The torch stand-in's tensors (synthetic runs take the same native path as checkpoints)."""
        if enc.dim % enc.heads or enc.dim // enc.heads != 64:
            raise NotImplementedError(f"head dimension {enc.dim / enc.heads:g} (dim {enc.dim} / heads {enc.heads}): "
                                      "the native text encoder implements 64 only")
        device = device if device is not None else (enc.tok.device if enc.tok.is_cuda else "cuda:0")
        return cls(enc.dim, len(enc.blocks), enc.heads, enc.tok.shape[0], enc.pos.shape[0], 0, None, device).load_state_dict(
            standin_to_clip_names(enc))

    # ------------------------------------------------------------------ the native handle
    def to(self, device):
        if torch.device(device) != self.device:
            self._native_release()
            self.device, self._ws = torch.device(device), None
        return self

    def eval(self):
        return self

    def _native(self):
        from . import _lib
        if self._h is not None:
            return self._h
        if self.params is None:
            raise RuntimeError("NativeClipText has no parameters: use one of the from_* loaders or load_state_dict")
        if self.device.type != "cuda":
            raise RuntimeError("NativeClipText runs on the HIP executor only (there is no CPU / torch path)")
        cfg = _lib.TextCfg(self.width, self.layers, self.heads, self.vocab_size, self.context_length, self.proj_dim)
        return self._native_build(self.device, self.params, cfg)

    def pool_index(self, input_ids):
        if self.eos_token_id is None:
            return input_ids.argmax(-1)
        return (input_ids == self.eos_token_id).int().argmax(-1)

    def __call__(self, input_ids, **unused):
        from . import _lib
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"input_ids: expected an integer (B, L) tensor, got {input_ids.dtype} {tuple(input_ids.shape)}")
        host = input_ids.detach().cpu()        # no copy and no synchronisation for host ids (what HEditEngine.encode passes)
        B, L = host.shape
        if B < 1 or L < 1:
            raise ValueError(f"input_ids: empty batch {tuple(host.shape)}")
        lo, hi = int(host.min()), int(host.max())
        if lo < 0 or hi >= self.vocab_size:
            raise ValueError(f"input_ids: token id {lo if lo < 0 else hi} outside [0, {self.vocab_size})")
        h = self._native()
        dev = self.device
        ids = host.to(torch.int32).to(dev).contiguous()
        pidx = self.pool_index(host).to(torch.int32).to(dev).contiguous()
        hidden = torch.empty(B, L, self.width, device=dev, dtype=torch.float32)
        pooled = torch.empty(B, self.proj_dim or self.width, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            need = self._need.get((B, L))
            if need is None:
                need = self._need[(B, L)] = self._lib.hedit_text_workspace_bytes(h, B, L)
            if need == 0:
                _lib.check(self._lib.hedit_text_encode(h, _lib.ptr(ids), B, L, _lib.ptr(hidden), _lib.ptr(pidx), _lib.ptr(pooled), None, 0,
                                                       _lib.cur_stream()))          # raises with the library's message
            self._grow("_ws", need, dev)
            _lib.check(self._lib.hedit_text_encode(h, _lib.ptr(ids), B, L, _lib.ptr(hidden), _lib.ptr(pidx), _lib.ptr(pooled),
                                                   _lib.ptr(self._ws), self._ws.numel(), _lib.cur_stream()))
        self.calls += 1
        return TextEncoderOutput(hidden, pooled)
