"""``MutualSelfAttentionControl`` -- mirrors text-guided/masactrl/masactrl.py:11-69.

Reference semantics (:53-69): in the self-attention of transformer block ``cur_att_layer // 2`` in
``layer_idx``, at editor step ``cur_step`` in ``step_idx``, the batch is split into its unconditional and
conditional halves and EVERY row of a half attends with its own queries to the keys and values of the
FIRST row of that half (the source image).  Here that is a per-row index handed to the self-attention
kernel (``hedit_p2p_plan.kv_src`` + ``kv_first_block``): no probabilities are materialised.  ``layer_idx``
must be a contiguous range up to the last block (what ``start_layer`` produces and the drivers use)."""
import torch

from .. import _lib
from .masactrl_utils import AttentionBase


class MutualSelfAttentionControl(AttentionBase):
    MODEL_TYPE = {"SD": 16, "SDXL": 70}

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, model_type="SD"):
        super().__init__()
        self.total_steps = total_steps
        self.total_layers = self.MODEL_TYPE.get(model_type, 16)
        self.start_step = start_step
        self.start_layer = start_layer
        self.layer_idx = layer_idx if layer_idx is not None else list(range(start_layer, self.total_layers))
        self.step_idx = step_idx if step_idx is not None else list(range(start_step, total_steps))
        if list(self.layer_idx) != list(range(min(self.layer_idx, default=self.total_layers), self.total_layers)):
            raise NotImplementedError("layer_idx must be range(k, total_layers) (the kernel gate is 'block >= k')")
        self._cache = {}

    def _plan(self, unet, B, H, W, save_attn):
        """B rows = [unconditional half | conditional half], each half laid out [source rows..., target rows...]
        with n images per kind (n = B / 4 in the h-Edit passes: [x_orig|null]*n, [x_k|null]*n, [x_orig|src]*n, [x_k|tar]*n):
        row (kind, i) reads the keys / values of row (first kind of its half, i)."""
        if B % 4:
            raise ValueError("a MasaCtrl pass expects [x_orig|null]*n, [x_edit|null]*n, [x_orig|src]*n, [x_edit|tar]*n rows")
        key = (id(unet), B)
        st = self._cache.get(key)
        if st is None:
            n = B // 4
            ar = torch.arange(B, dtype=torch.int32)
            kv = ar.clone()
            kv[n:2 * n] = ar[0:n]
            kv[3 * n:4 * n] = ar[2 * n:3 * n]
            st = (ar.to(unet.device), kv.to(unet.device))
            self._cache = {key: st}
        p = _lib.P2PPlan()
        p.mode = 1
        p.n_pairs = 0
        p.singles = st[0].data_ptr()
        p.n_single = B
        if self.cur_step in self.step_idx and len(self.layer_idx):
            p.kv_src = st[1].data_ptr()
            p.kv_first_block = int(min(self.layer_idx))
        p._keep = st
        return p


def _binary_masks(mask, name):
    """``(h, w)`` or ``(n, h, w)`` tensor with values in {0, 1} -> float32 ``(n, h, w)`` on the host (n = 1 for ``(h, w)``)"""
    m = torch.as_tensor(mask).detach().to("cpu", torch.float32)
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3:
        raise ValueError(f"{name} must have shape (h, w) or (n, h, w), got {tuple(m.shape)}")
    if not bool(((m == 0) | (m == 1)).all()):
        raise ValueError(f"{name} must hold only the values 0 and 1 (a soft mask has no class-matched form)")
    return m


def mask_classes(mask, res):
    """Class bytes of a binary ``(n, h, w)`` mask at a ``res x res`` layer, ``(n, res * res)`` uint8: the reference's
    ``F.interpolate(mask, (H, W))`` (default nearest, masactrl.py:104 / :142), flattened row-major like the tokens."""
    import torch.nn.functional as F
    return F.interpolate(mask[:, None], (res, res))[:, 0].reshape(mask.shape[0], res * res).to(torch.uint8)


def block_resolutions(unet, H):
    """side length of the token grid of every transformer block in call order (the index ``layer_idx`` counts), for an
    ``H x H`` latent: down blocks, the mid block, up blocks"""
    cfg = unet.config
    L, lpb = len(cfg["block_out_channels"]), cfg["layers_per_block"]
    res = []
    for lvl in range(L):
        if cfg["down_block_types"][lvl].startswith("CrossAttn"):
            res += [H >> lvl] * lpb
    res.append(H >> (L - 1))
    for j in range(L):
        if cfg["up_block_types"][j].startswith("CrossAttn"):
            res += [H >> (L - 1 - j)] * (lpb + 1)
    return res


def _write_mask_png(path, mask):
    """8-bit PNG of a (res, res) class array"""
    import numpy as np
    from PIL import Image
    Image.fromarray((np.asarray(mask, dtype=np.uint8) * 255)).save(path)


class _MaskedEditor(MutualSelfAttentionControl):
    """what the two mask-guided editors share: the 4n-row layout, the listed (target) rows, the refusals"""

    def _masked_plan(self, unet, B, H, W, save_attn, kw):
        name = type(self).__name__
        if kw:
            raise NotImplementedError(f"{name} runs in the 4n-row h-Edit passes only (a pass with {sorted(kw)} has no "
                                      "[source | target] x [null | prompt] row layout for the masks)")
        if H != W:
            raise NotImplementedError(f"{name}: non-square layer ({H} x {W}); the masks live on square layers")
        return super()._plan(unet, B, H, W, save_attn)

    @staticmethod
    def _listed_rows(unet, n):
        import ctypes as C
        listed = list(range(n, 2 * n)) + list(range(3 * n, 4 * n))
        return torch.tensor(listed, dtype=torch.int32, device=unet.device), (C.c_int32 * (2 * n))(*listed)

    def _active_blocks(self, unet, H):
        """[(block index, resolution)] of the blocks the editor is active in and the kernel can mask"""
        res = block_resolutions(unet, H)
        return [(b, res[b]) for b in self.layer_idx if b < len(res) and (res[b] * res[b]) % 64 == 0 and res[b] <= 64]


class MutualSelfAttentionControlMask(_MaskedEditor):
    """Mask-guided MasaCtrl with masks from the caller -- mirrors text-guided/masactrl/masactrl.py:71-148, the reference's
    argument order and defaults.

    Reference semantics: in an active layer the target rows attend to the source row's keys twice, once with the background
    keys filled with ``finfo.min`` and once with the foreground keys filled, and the two outputs are blended with the binary
    target mask.  With binary masks that is one softmax per query over the keys of the query's own class, which is what the
    class-matched kernel (``hedit_p2p_plan.masa_rows`` + class arrays) computes; a query whose class has no key gets the mean
    of V, the reference's fp32 result.  The source rows never see a mask.

    ``mask_s`` / ``mask_t``: ``(h, w)`` tensors with values in {0, 1}, one pair for both halves of the pass -- or ``(n, h, w)``,
    image i of a lock-step batch then gets mask i (an addition).  The reference's behaviour with ``mask_s=None``, or with
    ``mask_t=None`` beside a given ``mask_s``, is a shape-dependent accident and is refused.  ``mask_save_dir`` writes
    ``mask_s.png`` / ``mask_t.png`` (8-bit).  ``keep_masks=True`` (an addition) records the class arrays every active
    ``(step, layer)`` ran with: ``saved_masks[(step, layer)] = (source, target)``, ``(n, res, res)`` uint8 host tensors."""

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, mask_s=None, mask_t=None,
                 mask_save_dir=None, keep_masks=False):
        super().__init__(start_step, start_layer, layer_idx, step_idx, total_steps)
        if mask_s is None:
            raise ValueError("MutualSelfAttentionControlMask: mask_s is missing (use MutualSelfAttentionControl for the unmasked editor)")
        if mask_t is None:
            raise ValueError("MutualSelfAttentionControlMask: mask_t is missing (mask_s alone has no defined blend)")
        self.mask_s = _binary_masks(mask_s, "mask_s")
        self.mask_t = _binary_masks(mask_t, "mask_t")
        if self.mask_s.shape != self.mask_t.shape:
            raise ValueError(f"mask_s {tuple(self.mask_s.shape)} and mask_t {tuple(self.mask_t.shape)} must have the same shape")
        self.keep_masks = bool(keep_masks)
        self.saved_masks = {}
        self._mcache = {}
        if mask_save_dir is not None:
            import os
            os.makedirs(mask_save_dir, exist_ok=True)
            _write_mask_png(os.path.join(mask_save_dir, "mask_s.png"), self.mask_s[0].numpy())
            _write_mask_png(os.path.join(mask_save_dir, "mask_t.png"), self.mask_t[0].numpy())

    def _plan(self, unet, B, H, W, save_attn, **kw):
        p = self._masked_plan(unet, B, H, W, save_attn, kw)
        if not p.kv_src:
            return p
        n = B // 4
        if self.mask_s.shape[0] not in (1, n):
            raise ValueError(f"{self.mask_s.shape[0]} masks for {n} images: give one (h, w) pair or (n, h, w) masks")
        key = (id(unet), B, H, W)
        st = self._mcache.get(key)
        if st is None:
            import ctypes as C
            blocks = self._active_blocks(unet, H)
            res = sorted({r for _, r in blocks})
            ms, mt = (m.expand(n, -1, -1) for m in (self.mask_s, self.mask_t))
            host, dev = {}, []
            for r in res:
                cs, ct = mask_classes(ms, r), mask_classes(mt, r)             # (n, r * r)
                host[r] = (cs.reshape(n, r, r), ct.reshape(n, r, r))
                # row (kind, i): the source rows carry mask_s (read as key classes), the target rows mask_t (query classes)
                dev.append(torch.cat([cs, ct, cs, ct]).contiguous().to(unet.device))
            rows, h_rows = self._listed_rows(unet, n)
            h_cls = (C.c_void_p * len(res))(*[t.data_ptr() for t in dev])
            st = dict(blocks=blocks, host=host, dev=dev, rows=rows, h_rows=h_rows, h_cls=h_cls,
                      h_tok=(C.c_int32 * len(res))(*[r * r for r in res]))
            self._mcache = {key: st}
        if st["dev"]:
            p.masa_rows = st["rows"].data_ptr()
            p.h_masa_rows = st["h_rows"]
            p.n_masa_rows = 2 * n
            p.h_masa_cls_q = st["h_cls"]
            p.h_masa_cls_k = st["h_cls"]
            p.h_masa_tokens = st["h_tok"]
            p.n_masa_res = len(st["dev"])
        p._keep = (p._keep, st)
        if self.keep_masks:
            for b, r in st["blocks"]:
                self.saved_masks[(self.cur_step, b)] = st["host"][r]
        return p


class MutualSelfAttentionControlMaskAuto(_MaskedEditor):
    """Mask-guided MasaCtrl with masks from the pass's own cross-attention maps -- mirrors
    text-guided/masactrl/masactrl.py:151-286, the reference's argument order and defaults.

    Per UNet pass the executor folds the head-mean probabilities of every 256-token cross-attention layer into an accumulator
    (the columns ``ref_token_idx`` on the conditional source row, ``cur_token_idx`` on the conditional target row).  At an
    active self-attention layer the mean over the layers collected so far in this pass is min-max normalised per image, taken
    nearest from 16 x 16 to the layer's resolution and thresholded ``>= thres``: the source map masks the keys, the target
    map the queries.  While no map has been collected the layer runs unmasked mutual attention (:247-250).  A constant map
    gives class 0 everywhere (the reference divides 0 by 0 there).  Nothing waits for the device.

    ``mask_save_dir`` writes ``mask_s_{step}_{layer}.png`` / ``mask_t_{step}_{layer}.png`` (``layer`` = the attention-layer
    counter as in the reference, twice the block index; the thresholded masks, 8-bit); ``keep_masks=True`` (an addition) keeps
    the same arrays in ``saved_masks[(step, block)] = (source, target)``, ``(n, res, res)`` uint8 host tensors.  Either one
    copies the masks to the host after the pass; without them nothing leaves the device."""

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, thres=0.1,
                 ref_token_idx=[1], cur_token_idx=[1], mask_save_dir=None, keep_masks=False):
        super().__init__(start_step, start_layer, layer_idx, step_idx, total_steps)
        self.thres = float(thres)
        self.ref_token_idx = [int(t) for t in (ref_token_idx if isinstance(ref_token_idx, (list, tuple)) else [ref_token_idx])]
        self.cur_token_idx = [int(t) for t in (cur_token_idx if isinstance(cur_token_idx, (list, tuple)) else [cur_token_idx])]
        for name, idx in (("ref_token_idx", self.ref_token_idx), ("cur_token_idx", self.cur_token_idx)):
            if not idx or min(idx) < 0 or max(idx) >= 77:
                raise ValueError(f"{name} must list token positions in [0, 77), got {idx}")
        self.mask_save_dir = mask_save_dir
        if mask_save_dir is not None:
            import os
            os.makedirs(mask_save_dir, exist_ok=True)
        self.keep_masks = bool(keep_masks)
        self.saved_masks = {}
        self._mcache = {}
        self._pending = None

    def _plan(self, unet, B, H, W, save_attn, **kw):
        p = self._masked_plan(unet, B, H, W, save_attn, kw)
        self._pending = None
        if not p.kv_src:
            return p
        n = B // 4
        key = (id(unet), B, H, W)
        st = self._mcache.get(key)
        if st is None:
            heads = unet.config["attention_head_dim"]
            ws_bytes = 2 * n * 256 * 4 + 4 * n * 4096 + 2 * n * heads * 256 * 77 * 4
            rows, h_rows = self._listed_rows(unet, n)
            st = dict(rows=rows, h_rows=h_rows, ws=torch.empty(ws_bytes, dtype=torch.uint8, device=unet.device), ws_bytes=ws_bytes,
                      ref=torch.tensor(self.ref_token_idx, dtype=torch.int32, device=unet.device),
                      cur=torch.tensor(self.cur_token_idx, dtype=torch.int32, device=unet.device),
                      res=block_resolutions(unet, H))
            self._mcache = {key: st}
        p.masa_rows = st["rows"].data_ptr()
        p.h_masa_rows = st["h_rows"]
        p.n_masa_rows = 2 * n
        p.masa_auto = 1
        p.masa_thres = self.thres
        p.masa_images = n
        p.masa_ref_tokens = st["ref"].data_ptr()
        p.n_masa_ref = len(self.ref_token_idx)
        p.masa_cur_tokens = st["cur"].data_ptr()
        p.n_masa_cur = len(self.cur_token_idx)
        p.masa_ws = st["ws"].data_ptr()
        p.masa_ws_bytes = st["ws_bytes"]
        keep = [p._keep, st]
        if self.keep_masks or self.mask_save_dir is not None:
            import ctypes as C
            first = int(min(self.layer_idx))
            res = st["res"][first:]                         # the layers under kv_src, in call order
            # 255 = "this layer ran unmasked" (no map collected yet, or a token count the kernel does not take)
            dumps = [torch.full((B, r * r), 255, dtype=torch.uint8, device=unet.device) for r in res]
            h_dump = (C.c_void_p * max(len(dumps), 1))(*[t.data_ptr() for t in dumps])
            p.h_masa_dump = h_dump
            p.n_masa_dump = len(dumps)
            keep += [dumps, h_dump]
            self._pending = (self.cur_step, first, n, res, dumps)
        p._keep = tuple(keep)
        return p

    def _after_pass(self, save_attn):
        pend, self._pending = self._pending, None
        if pend is not None:
            step, first, n, res, dumps = pend
            for j, (r, t) in enumerate(zip(res, dumps)):
                m = t.cpu()
                if int(m[0, 0]) == 255:
                    continue
                src, tar = m[2 * n:3 * n].reshape(n, r, r), m[3 * n:4 * n].reshape(n, r, r)
                if self.keep_masks:
                    self.saved_masks[(step, first + j)] = (src, tar)
                if self.mask_save_dir is not None:
                    import os
                    layer = 2 * (first + j)
                    _write_mask_png(os.path.join(self.mask_save_dir, f"mask_s_{step}_{layer}.png"), src[0].numpy())
                    _write_mask_png(os.path.join(self.mask_save_dir, f"mask_t_{step}_{layer}.png"), tar[0].numpy())
        super()._after_pass(save_attn)
