"""fp64 restatement of the reference's two mask-guided MasaCtrl editors (text-guided/masactrl/masactrl.py:71-148 and
:151-286) as attention processors for the oracle UNets -- they plug in through ``set_attn_processor`` the way
``oracle.masactrl.MasaProcessor`` does.  PINNED on vectors from running the reference's own classes
(tests/golden/g28_masactrl_mask.npz, written by tests/golden/make_golden_masactrl_mask.py).

Written as the reference computes it: per target row TWO softmaxes over the source row's keys -- foreground keys kept
(mask value 1 added to their logits) and background keys filled with ``finfo.min``, and the other way round -- then the
blend of the two outputs with the target mask.  A query whose class has no key sees ``sim + finfo.min`` everywhere, which
absorbs ``sim``: the uniform softmax, the mean of V.  The one-softmax form is what the HIP kernel is tested AGAINST."""
import torch
import torch.nn.functional as F

from oracle import masactrl as OM


# ------------------------------------------------------------------------------------------------ the arithmetic
def attend(q, k, v, scale):
    """(h, n, d) each -> (n, h * d)"""
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
    return (p @ v).transpose(0, 1).reshape(q.shape[1], -1)


def attend_masked(q, k, v, scale, mask_s, mask_t):
    """target queries q on the source's k, v (h, n, d); mask_s / mask_t: flat (n,) tensors of 0 / 1 in q's dtype"""
    sim = q @ k.transpose(-1, -2) * scale                                   # (h, n, n)
    lo = torch.finfo(sim.dtype).min
    sim_fg = sim + mask_s.masked_fill(mask_s == 0, lo)
    sim_bg = sim + mask_s.masked_fill(mask_s == 1, lo)
    out_fg = (torch.softmax(sim_fg, -1) @ v).transpose(0, 1).reshape(q.shape[1], -1)
    out_bg = (torch.softmax(sim_bg, -1) @ v).transpose(0, 1).reshape(q.shape[1], -1)
    m = mask_t.reshape(-1, 1)
    return out_fg * m + out_bg * (1 - m)


def at_resolution(mask, res):
    """(h, w) -> flat (res * res,): the reference's F.interpolate(mask[None, None], (res, res)), default nearest"""
    return F.interpolate(mask[None, None], (res, res)).flatten()


def aggregate(cross, idx):
    """the reference's aggregate_cross_attn_map (:212-223): cross = list of (b, 256, 77) head-mean maps -> (b, 16, 16),
    columns idx summed, min-max normalised per image (a constant map divides 0 by 0, as there)"""
    m = torch.stack(cross, dim=1).mean(1)
    res = int(round(m.shape[-2] ** 0.5))
    img = m.reshape(-1, res, res, m.shape[-1])[..., list(idx)].sum(-1)
    lo = img.amin(dim=(1, 2), keepdim=True)
    hi = img.amax(dim=(1, 2), keepdim=True)
    return (img - lo) / (hi - lo)


def auto_masks(cross, ref_idx, cur_idx, thres, res, constant_is_background=False):
    """binarised (mask_s, mask_t), flat (res * res,), from the conditional source row ([-2], ref tokens) and the conditional
    target row ([-1], cur tokens); also the normalised maps before the threshold.  constant_is_background: what the HIP
    path does with a constant map (class 0 everywhere) where the reference has NaN"""
    ns = at_resolution(aggregate(cross, ref_idx)[-2], res)
    nt = at_resolution(aggregate(cross, cur_idx)[-1], res)
    if constant_is_background:
        ns, nt = torch.nan_to_num(ns, nan=-1.0), torch.nan_to_num(nt, nan=-1.0)
    return (ns >= thres).to(ns.dtype), (nt >= thres).to(nt.dtype), ns, nt


def editor_rows(q, k, v, scale, masks):
    """One active self-attention layer on the reference's 4 rows [x_orig|null, x_k|null, x_orig|src, x_k|tar]: q, k, v
    (4, h, n, d).  masks = (mask_s, mask_t) flat, or None (unmasked mutual attention).  -> (4, n, h * d)"""
    out = []
    for b in range(4):
        s = 0 if b < 2 else 2
        if b in (0, 2) or masks is None:
            out.append(attend(q[b], k[s], v[s], scale))
        else:
            out.append(attend_masked(q[b], k[s], v[s], scale, masks[0], masks[1]))
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------ seeded inputs of the golden file
def golden_qkv(seed, heads, d, N):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(4, heads, N, d, generator=g) for _ in range(3))


def golden_cross(seed, heads, layers=3):
    """`layers` fake cross-attention probability tensors (4, heads, 256, 77), peaked enough to give structured maps"""
    g = torch.Generator().manual_seed(seed)
    return [torch.softmax(2.0 * torch.randn(4, heads, 256, 77, generator=g), dim=-1) for _ in range(layers)]


def golden_given_masks(kind, seed, size=32):
    g = torch.Generator().manual_seed(seed)
    if kind == "mixed":
        return (torch.rand(size, size, generator=g) < 0.5).float(), (torch.rand(size, size, generator=g) < 0.5).float()
    if kind == "empty":                      # source all foreground: the background queries of the target have no key
        return torch.ones(size, size), (torch.rand(size, size, generator=g) < 0.5).float()
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------ editors and processor
class MaskEditor(OM.MutualSelfAttention):
    """mode 'given': mask_s / mask_t (h, w); 'auto': thres / ref_idx / cur_idx, maps from the pass's 256-token cross layers;
    'replay': masks[(step, block)] = (mask_s, mask_t) (res, res) arrays taken as they are (a block without an entry runs
    unmasked mutual attention)."""

    def __init__(self, start_step=4, start_layer=10, total_steps=50, total_layers=16, mode="given", mask_s=None, mask_t=None,
                 thres=0.1, ref_idx=(1,), cur_idx=(1,), masks=None):
        super().__init__(start_step, start_layer, total_steps, total_layers)
        self.mode, self.mask_s, self.mask_t = mode, mask_s, mask_t
        self.thres, self.ref_idx, self.cur_idx, self.masks = thres, tuple(ref_idx), tuple(cur_idx), masks
        self.cross = []
        self.used = {}                       # (step, block) -> (mask_s, mask_t) the layer ran with

    def count(self):
        step = self.cur_step
        super().count()
        if self.cur_step != step:
            self.cross = []                  # after_step (:182-184)

    def masks_for(self, res, dtype):
        key = (self.cur_step, self.cur_att_layer // 2)
        if self.mode == "given":
            m = at_resolution(self.mask_s.to(dtype), res), at_resolution(self.mask_t.to(dtype), res)
        elif self.mode == "auto":
            if not self.cross:
                return None
            m = auto_masks(self.cross, self.ref_idx, self.cur_idx, self.thres, res, constant_is_background=True)[:2]
        else:
            got = self.masks.get(key)
            if got is None:
                return None
            m = tuple(torch.as_tensor(x).to(dtype).reshape(-1) for x in got)
        self.used[key] = m
        return m


class MaskProcessor:
    def __init__(self, editor):
        self.editor = editor

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, use_editor=True):
        x = hidden_states
        is_cross = encoder_hidden_states is not None
        ctx = encoder_hidden_states if is_cross else x
        h = attn.heads
        b, n, c = x.shape
        ed = self.editor
        q = attn.to_q(x).reshape(b, n, h, c // h).transpose(1, 2).double()
        k = attn.to_k(ctx).reshape(b, ctx.shape[1], h, c // h).transpose(1, 2).double()
        v = attn.to_v(ctx).reshape(b, ctx.shape[1], h, c // h).transpose(1, 2).double()
        if use_editor and is_cross and n == 256 and ed.mode == "auto":
            ed.cross.append(torch.softmax(q @ k.transpose(-1, -2) * attn.scale, dim=-1).mean(1))     # (b, 256, 77)
        if use_editor and ed.active(is_cross):
            assert b == 4, "the restatement covers the reference's 4-row pass"
            o = editor_rows(q, k, v, attn.scale, ed.masks_for(int(round(n ** 0.5)), q.dtype))
        else:
            o = (torch.softmax(q @ k.transpose(-1, -2) * attn.scale, dim=-1) @ v).transpose(1, 2).reshape(b, n, c)
        if use_editor:
            ed.count()
        to_out = attn.to_out[0] if isinstance(attn.to_out, torch.nn.ModuleList) else attn.to_out
        return to_out(o.to(x.dtype))


def register_editor(model, editor):
    procs = {name: MaskProcessor(editor) for name in model.unet.attn_processors.keys()}
    model.unet.set_attn_processor(procs)
    editor.num_att_layers = len(procs)
