"""CLIP score on the native executors: the image tower (``hedit_clipimg_*`` of libhedit_hip.so, csrc/clipimg.hip), the
text tower (``hedit_text_*``, csrc/text.hip) and the metric the PIE-Bench evaluator reports in its ``clip_similarity_*``
columns -- torchmetrics' ``CLIPScore(model_name_or_path="openai/clip-vit-large-patch14")`` of the reference's
text-guided/evaluation/matrics_calculator.py:274,290-302: ``max(100 * cos(image embedding, text embedding), 0)``.

Nothing here is ever fetched: models come from local files (a transformers-style directory or an OpenAI ``.pt``) or from
seeded stand-in weights, and there is no torch forward -- without the library the classes raise.
"""
import json
import os

import numpy as np
import torch

from .native import NativeOwner
from .text import NativeClipText, _cfg_get

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_TOKENS = 577          # csrc/clipimg.hip: ViT-L/14@336
MAX_BATCH = 256           # HEDIT_CLIPIMG_MAX_BATCH of include/hedit.h

_BLOCK_SHAPES = (("ln_1.weight", (1,)), ("ln_1.bias", (1,)), ("attn.in_proj_weight", (3, 1)), ("attn.in_proj_bias", (3,)),
                 ("attn.out_proj.weight", (1, 1)), ("attn.out_proj.bias", (1,)), ("ln_2.weight", (1,)), ("ln_2.bias", (1,)),
                 ("mlp.c_fc.weight", (4, 1)), ("mlp.c_fc.bias", (4,)), ("mlp.c_proj.weight", (1, 4)), ("mlp.c_proj.bias", (1,)))
# transformers CLIPVisionModel -> OpenAI CLIP, per layer (q / k / v are concatenated in that order into in_proj_*)
_HF_BLOCK = (("layer_norm1", "ln_1"), ("self_attn.out_proj", "attn.out_proj"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
             ("mlp.fc2", "mlp.c_proj"))
_HF_TOP = (("embeddings.class_embedding", "visual.class_embedding"), ("embeddings.patch_embedding.weight", "visual.conv1.weight"),
           ("embeddings.position_embedding.weight", "visual.positional_embedding"),
           ("pre_layrnorm.weight", "visual.ln_pre.weight"), ("pre_layrnorm.bias", "visual.ln_pre.bias"),      # (sic) transformers' spelling
           ("post_layernorm.weight", "visual.ln_post.weight"), ("post_layernorm.bias", "visual.ln_post.bias"))


def clipimg_param_shapes(width, layers, patch_size, input_resolution, embed_dim):
    """The native executor's parameter table (csrc/clipimg.hip: OpenAI CLIP state_dict names), name -> shape, in its order."""
    tokens = (input_resolution // patch_size) ** 2 + 1
    out = {"visual.conv1.weight": (width, 3, patch_size, patch_size), "visual.class_embedding": (width,),
           "visual.positional_embedding": (tokens, width), "visual.ln_pre.weight": (width,), "visual.ln_pre.bias": (width,)}
    for i in range(layers):
        for name, mult in _BLOCK_SHAPES:
            out[f"visual.transformer.resblocks.{i}.{name}"] = tuple(m * width for m in mult)
    out["visual.ln_post.weight"] = (width,)
    out["visual.ln_post.bias"] = (width,)
    out["visual.proj"] = (width, embed_dim)
    return out


def hf_vision_to_clip_names(sd, layers):
    """transformers CLIPModel / CLIPVisionModelWithProjection names (``vision_model.*`` + ``visual_projection.weight``) ->
    OpenAI CLIP names.  Entries of the text tower and ``logit_scale`` are dropped; any other key this function does not know
    is passed through under its own name, so the strict check of the caller reports it as unexpected."""
    sd = {k: v for k, v in sd.items() if not k.startswith(("text_model.", "text_projection.")) and k != "logit_scale"}
    sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}
    sd.pop("embeddings.position_ids", None)              # an index buffer older checkpoints persist, not a parameter
    out, used = {}, set()

    def take(src, dst):
        if src in sd:
            out[dst] = sd[src]
            used.add(src)

    for a, b in _HF_TOP:
        take(a, b)
    if "visual_projection.weight" in sd:                 # nn.Linear [embed][width], no bias; CLIP multiplies by [width][embed]
        out["visual.proj"] = sd["visual_projection.weight"].t().contiguous()
        used.add("visual_projection.weight")
    for i in range(layers):
        src, dst = f"encoder.layers.{i}.", f"visual.transformer.resblocks.{i}."
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


def preprocess_pil(img, size):
    """What transformers' CLIPImageProcessor does to one RGB image (PIL image or uint8 H x W x 3 array): shortest edge to
    `size` with PIL bicubic (the long edge ``int(size * long / short)``), centre crop to size x size, ``/ 255`` (in float64,
    rounded to float32, as the processor rescales), CLIP mean and std in float32.  -> float32 array [3][size][size]."""
    from PIL import Image
    if not isinstance(img, Image.Image):
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"preprocess_pil: expected a PIL image or a uint8 (H, W, 3) array, got {a.dtype} {a.shape}")
        img = Image.fromarray(a)
    img = img.convert("RGB")
    w, h = img.size
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = int(size), int(size * long / short)
    nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    a = np.array(img.resize((nw, nh), resample=Image.BICUBIC))
    top, left = (nh - size) // 2, (nw - size) // 2
    a = a[top:top + size, left:left + size].transpose(2, 0, 1)
    x = (a.astype(np.float64) * (1 / 255)).astype(np.float32)
    mean = np.array(CLIP_MEAN, dtype=np.float32)[:, None, None]
    std = np.array(CLIP_STD, dtype=np.float32)[:, None, None]
    return (x - mean) / std


class NativeClipImage(NativeOwner):
    """The CLIP image tower on the native executor: a parameter container under the OpenAI CLIP names plus the native
    handle.  There is no torch forward.  ``model(pixel_values)`` -> (B, embed_dim) fp32, not normalised; results are
    bit-identical whatever the batch (``batch_invariant``)."""
    batch_invariant = True
    _family = "clipimg"

    def __init__(self, width, layers, heads, patch_size, input_resolution, embed_dim, device="cuda:0"):
        if width % heads or width // heads != 64:
            raise NotImplementedError(f"the native image tower has head dimension 64, not {width}/{heads} (width/heads)")
        if input_resolution % patch_size:
            raise NotImplementedError(f"input_resolution {input_resolution} is not a multiple of patch_size {patch_size}")
        tokens = (input_resolution // patch_size) ** 2 + 1
        if tokens > MAX_TOKENS:
            raise NotImplementedError(f"{tokens} tokens ({input_resolution} px / patch {patch_size}): the native image tower takes at most {MAX_TOKENS}")
        if embed_dim % 4:
            raise NotImplementedError(f"visual.proj with {embed_dim} columns: the native image tower needs a multiple of 4")
        self.width, self.layers, self.heads = int(width), int(layers), int(heads)
        self.patch_size, self.input_resolution, self.embed_dim, self.tokens = int(patch_size), int(input_resolution), int(embed_dim), tokens
        self.device = torch.device(device)
        self.param_shapes = clipimg_param_shapes(self.width, self.layers, self.patch_size, self.input_resolution, self.embed_dim)
        self.params = None
        self.calls = 0                # native encode calls made (tests count them)
        self._need = {}
        self._slices = 0

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
    def from_clip_state_dict(cls, sd, device="cuda:0"):
        """A full OpenAI CLIP state_dict (e.g. a local ViT-L-14.pt read with ``base_clip.read_clip_checkpoint``): the
        ``visual.*`` entries are the image tower's, everything else is ignored."""
        sd = {k: v for k, v in sd.items() if k.startswith("visual.")}
        for k in ("visual.conv1.weight", "visual.positional_embedding", "visual.proj"):
            if k not in sd:
                raise KeyError(f"state_dict mismatch: missing ['{k}'] (1), unexpected [] (0)")
        if sd["visual.conv1.weight"].dim() != 4 or "visual.layer1.0.conv1.weight" in sd:
            raise NotImplementedError("the native image tower implements CLIP's vision transformers, not its ResNets")
        width, _, patch, _ = sd["visual.conv1.weight"].shape
        grid = int(round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5))
        layers = len({k.split(".")[3] for k in sd if k.startswith("visual.transformer.resblocks.")})
        if width % 64:
            raise NotImplementedError(f"the native image tower has head dimension 64; width {width} is not a multiple of it")
        return cls(width, layers, width // 64, patch, grid * patch, sd["visual.proj"].shape[1], device).load_state_dict(sd)

    @staticmethod
    def check_hf_config(config):
        """(hidden_size, heads) of a transformers vision config this executor implements, else NotImplementedError by name"""
        act = _cfg_get(config, "hidden_act", "quick_gelu")
        if act != "quick_gelu":
            raise NotImplementedError(f"hidden_act {act!r}: the native image tower implements quick_gelu only")
        width, heads = int(_cfg_get(config, "hidden_size")), int(_cfg_get(config, "num_attention_heads"))
        if width % heads or width // heads != 64:
            raise NotImplementedError(f"head dimension {width / heads:g} (hidden_size {width} / num_attention_heads {heads}): "
                                      "the native image tower implements 64 only")
        return width, heads

    @classmethod
    def from_hf_state_dict(cls, sd, config, projection_dim=None, device="cuda:0"):
        """transformers CLIPModel / CLIPVisionModelWithProjection weights + the vision config (a dict, e.g. ``vision_config``
        of config.json, or a CLIPVisionConfig).  ``projection_dim`` defaults to the config's."""
        width, heads = cls.check_hf_config(config)
        layers = int(_cfg_get(config, "num_hidden_layers"))
        mapped = hf_vision_to_clip_names(sd, layers)
        embed = int(projection_dim if projection_dim is not None else
                    (mapped["visual.proj"].shape[1] if "visual.proj" in mapped else _cfg_get(config, "projection_dim")))
        return cls(width, layers, heads, int(_cfg_get(config, "patch_size")), int(_cfg_get(config, "image_size")), embed,
                   device).load_state_dict(mapped)

    @classmethod
    def from_standin(cls, width=1024, layers=24, heads=16, patch_size=14, input_resolution=224, embed_dim=768, seed=7, device="cuda:0"):
        """Seeded random weights for synthetic runs, generated on `device` (1.2 GB at the ViT-L/14 default)."""
        self = cls(width, layers, heads, patch_size, input_resolution, embed_dim, device)
        g = torch.Generator(device=self.device).manual_seed(seed)
        sd = {}
        for name, shape in self.param_shapes.items():
            if name.endswith(("ln_1.weight", "ln_2.weight", "ln_pre.weight", "ln_post.weight")):
                sd[name] = torch.ones(shape, device=self.device)
            elif name.endswith(".bias"):
                sd[name] = torch.zeros(shape, device=self.device)
            else:
                fan_in = width if len(shape) < 2 or name == "visual.proj" else int(np.prod(shape[1:]))
                sd[name] = torch.randn(shape, generator=g, device=self.device) * fan_in ** -0.5
        return self.load_state_dict(sd)

    # ------------------------------------------------------------------ the native handle
    def to(self, device):
        if torch.device(device) != self.device:
            self._native_release()
            self.device, self._ws = torch.device(device), None
        return self

    def eval(self):
        return self

    def set_slices(self, slices):
        """The slice count of the attention grid (0: one workgroup per 32-row pass).  It sizes the grid only; tests check that the
        output bits do not depend on it."""
        self._slices = int(slices)
        if self._h is not None:
            from . import _lib
            _lib.check(self._lib.hedit_clipimg_set_slices(self._h, self._slices))
        return self

    def _native(self):
        from . import _lib
        if self._h is not None:
            return self._h
        if self.params is None:
            raise RuntimeError("NativeClipImage has no parameters: use one of the from_* loaders or load_state_dict")
        if self.device.type != "cuda":
            raise RuntimeError("NativeClipImage runs on the HIP executor only (there is no CPU / torch path)")
        cfg = _lib.ClipImgCfg(self.width, self.layers, self.heads, self.patch_size, self.input_resolution, self.embed_dim)
        return self._native_build(self.device, self.params, cfg,
                                  after=lambda lib, h: _lib.check(lib.hedit_clipimg_set_slices(h, self._slices)))

    def __call__(self, pixel_values):
        from . import _lib
        R = self.input_resolution
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, R, R) or not pixel_values.is_floating_point():
            raise ValueError(f"pixel_values: expected a float (B, 3, {R}, {R}) tensor, got {pixel_values.dtype} {tuple(pixel_values.shape)}")
        B = pixel_values.shape[0]
        if B < 1 or B > MAX_BATCH:
            raise ValueError(f"pixel_values: batch {B} outside [1, {MAX_BATCH}]")
        h = self._native()
        dev = self.device
        x = pixel_values.detach().to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty(B, self.embed_dim, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            need = self._need.get(B)
            if need is None:
                need = self._need[B] = self._lib.hedit_clipimg_workspace_bytes(h, B)
            if need == 0:
                _lib.check(self._lib.hedit_clipimg_encode(h, _lib.ptr(x), B, _lib.ptr(out), None, 0, _lib.cur_stream()))   # raises with the library's message
            self._grow("_ws", need, dev)
            _lib.check(self._lib.hedit_clipimg_encode(h, _lib.ptr(x), B, _lib.ptr(out), _lib.ptr(self._ws), self._ws.numel(), _lib.cur_stream()))
        self.calls += 1
        return out


def _cosines(img, txt):
    """cos(img[i], txt[i]) in float64 on the host, one row at a time: a row's value cannot depend on the other rows"""
    a, b = img.detach().cpu().double().numpy(), txt.detach().cpu().double().numpy()
    return [float(np.dot(x, y) / (np.sqrt(np.dot(x, x)) * np.sqrt(np.dot(y, y)))) for x, y in zip(a, b)]


class NativeClip:
    """Image tower + text tower (``proj_dim = embed_dim``) + tokenizer: the two embeddings and the CLIP score.

    ``tokenizer``: anything with ``encode(text) -> [BOS, ..., EOS]`` ids and ``eos_token_id`` (transformers' CLIPTokenizer,
    ``hedit.text.WordTokenizer``)."""

    def __init__(self, image, text, tokenizer):
        if text.proj_dim != image.embed_dim:
            raise ValueError(f"text_projection has {text.proj_dim} columns, visual.proj {image.embed_dim}: not one embedding space")
        self.image, self.text, self.tokenizer = image, text, tokenizer
        self.native_preprocess = False        # pixel_values on the device (hedit.image_prep) instead of preprocess_pil
        self._prep = None

    # ------------------------------------------------------------------ loaders (local files only)
    @classmethod
    def from_pretrained(cls, path, device="cuda:0"):
        """A local ``openai/clip-vit-large-patch14``-style directory: config.json, model.safetensors or pytorch_model.bin,
        and the tokenizer files (read with transformers' CLIPTokenizer, ``local_files_only``).  Nothing is fetched."""
        cfg_path = os.path.join(path, "config.json")
        if not os.path.isfile(cfg_path):
            raise FileNotFoundError(f"{cfg_path}: not a CLIP model directory (for a bare OpenAI .pt use from_openai_checkpoint)")
        with open(cfg_path) as f:
            cfg = json.load(f)
        st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
        if os.path.isfile(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        elif os.path.isfile(pt):
            sd = torch.load(pt, map_location="cpu", weights_only=True)
        else:
            raise FileNotFoundError(f"{path}: neither model.safetensors nor pytorch_model.bin")
        vcfg, tcfg = cfg.get("vision_config") or {}, cfg.get("text_config") or {}
        for name, c in (("vision_config", vcfg), ("text_config", tcfg)):
            for k in ("hidden_size", "num_attention_heads", "num_hidden_layers"):
                if k not in c:
                    raise KeyError(f"{cfg_path}: {name}.{k} is missing")
        image = NativeClipImage.from_hf_state_dict(sd, vcfg, device=device)
        tsd = {k: v for k, v in sd.items() if k.startswith(("text_model.", "text_projection."))}
        text = NativeClipText.from_hf_state_dict(tsd, tcfg, device=device)
        from transformers import CLIPTokenizer
        return cls(image, text, CLIPTokenizer.from_pretrained(path, local_files_only=True))

    @classmethod
    def from_openai_checkpoint(cls, path, tokenizer_dir, device="cuda:0"):
        """A bare OpenAI CLIP file (ViT-L-14.pt: TorchScript archive or state_dict) + a local directory with the tokenizer files."""
        from .clip_guidance.base_clip import read_clip_checkpoint
        sd = read_clip_checkpoint(path)
        from transformers import CLIPTokenizer
        tok = CLIPTokenizer.from_pretrained(tokenizer_dir, local_files_only=True)
        return cls(NativeClipImage.from_clip_state_dict(sd, device=device),
                   NativeClipText.from_clip_state_dict(sd, device=device, eos_token_id=tok.eos_token_id), tok)

    @classmethod
    def from_standin(cls, width=1024, layers=24, heads=16, patch_size=14, input_resolution=224, embed_dim=768, text_width=768, text_layers=12,
                     seed=7, device="cuda:0"):
        """Seeded stand-in weights (ViT-L/14 shapes by default) and the word-level stand-in tokenizer: synthetic runs take
        the same native path as checkpoints."""
        from .text import WordTokenizer
        image = NativeClipImage.from_standin(width, layers, heads, patch_size, input_resolution, embed_dim, seed, device)
        tok = WordTokenizer(stable_ids=True)
        dev = image.device
        g = torch.Generator(device=dev).manual_seed(seed + 1)
        text = NativeClipText(text_width, text_layers, text_width // 64, tok.vocab_size, tok.model_max_length, embed_dim, tok.eos_token_id, dev)
        sd = {}
        for name, shape in text.param_shapes.items():
            if name.endswith(("ln_1.weight", "ln_2.weight", "ln_final.weight")):
                sd[name] = torch.ones(shape, device=dev)
            elif name.endswith("bias"):
                sd[name] = torch.zeros(shape, device=dev)
            else:
                scale = 0.02 if name == "token_embedding.weight" else (0.01 if name == "positional_embedding" else
                                                                       (shape[0] if name == "text_projection" else shape[1]) ** -0.5)
                sd[name] = torch.randn(shape, generator=g, device=dev) * scale
        return cls(image, text.load_state_dict(sd), tok)

    # ------------------------------------------------------------------ embeddings
    def tokenize(self, prompts):
        """(B, context_length) int64 ids: BOS, tokens, EOS, then padding with the EOS id.  A prompt longer than the context is
        cut and its last position set to the EOS, as CLIPProcessor truncates.  The text tower is causal (text.hip's prefix
        property: position i depends on the tokens 0..i alone), so whatever follows the first EOS cannot change the EOS row
        the embedding is read from -- the padding id is immaterial, and every call uses the full context length so that a
        prompt's bits do not depend on its neighbours' lengths."""
        L, eos = self.text.context_length, int(self.tokenizer.eos_token_id)
        rows = []
        for p in prompts:
            ids = [int(i) for i in self.tokenizer.encode(p)]
            if len(ids) > L:
                ids = ids[:L - 1] + [eos]
            rows.append(ids + [eos] * (L - len(ids)))
        return torch.tensor(rows, dtype=torch.int64)

    def text_features(self, prompts):
        """(B, embed_dim) fp32, not normalised; ONE native call for the whole list"""
        if isinstance(prompts, str):
            prompts = [prompts]
        ids = self.tokenize(prompts)
        eos = int(self.tokenizer.eos_token_id)
        first = (ids == eos).int().argmax(-1)
        if not torch.equal(self.text.pool_index(ids), first):
            raise ValueError("the text tower's pooling rule does not pick the first EOS of these ids: construct it with the "
                             f"tokenizer's eos_token_id ({eos})")
        return self.text(ids)[1]

    def pixel_values(self, images, native=None):
        """(B, 3, R, R) fp32: every PIL image / uint8 (H, W, 3) array through ``preprocess_pil``; a float (3, R, R) tensor is
        taken as already preprocessed.  ``native`` (default: ``self.native_preprocess``, False): the same values computed on
        the image tower's device by ``hedit.image_prep`` (its transformers convention: bit for bit ``preprocess_pil``'s), one
        upload and one native call per image size; the tensor then lives on that device."""
        R = self.image.input_resolution
        if not (self.native_preprocess if native is None else native):
            return torch.stack([im.detach().float().cpu() if torch.is_tensor(im) and im.is_floating_point() else
                                torch.from_numpy(preprocess_pil(im, R)) for im in images])
        from .image_prep import NativeImagePrep, image_u8
        dev = self.image.device
        if self._prep is None or self._prep.device != dev:
            self._prep = NativeImagePrep(dev)
        out, by_size = [None] * len(images), {}
        for i, im in enumerate(images):
            if torch.is_tensor(im) and im.is_floating_point():
                out[i] = im.detach().float().to(dev)
            else:
                a = image_u8(im)
                by_size.setdefault(a.shape, []).append((i, a))
        for group in by_size.values():
            for (i, _), x in zip(group, self._prep([a for _, a in group], R, "transformers")):
                out[i] = x
        return torch.stack(out)

    def image_features(self, images):
        """(B, embed_dim) fp32, not normalised; ONE native call for the whole list of PIL images / uint8 (H, W, 3) arrays /
        preprocessed float (3, R, R) tensors"""
        if not isinstance(images, (list, tuple)):
            images = [images]
        return self.image(self.pixel_values(images))

    # ------------------------------------------------------------------ the metric
    def scores(self, images, texts):
        """[max(100 cos(image_i, text_i), 0)]: torchmetrics' CLIPScore per sample.  Two native calls for the whole list;
        by batch invariance the values are those of the ``score`` loop bit for bit."""
        if len(images) != len(texts):
            raise ValueError(f"{len(images)} images for {len(texts)} texts")
        cos = _cosines(self.image_features(list(images)), self.text_features(list(texts)))
        return [max(100.0 * c, 0.0) for c in cos]

    def score(self, image, text):
        return self.scores([image], [text])[0]
