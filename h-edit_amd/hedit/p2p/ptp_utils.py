"""Registration + schedule tables of the P2P plug-in (host side).

Mirrors the parts of text-guided/p2p/ptp_utils.py that are on the h-Edit path:
P2PCrossAttnProcessor (:31-122), register_attention_control (:277-295), get_word_inds (:297-315),
update_alpha_time_word (:318-328), get_time_words_attention_alpha (:331-349).  The attention body
of the processor is NOT here: it runs inside the HIP kernels (csrc/attn.hip); the processor object
only tells the UNet which controller drives the edit and where the layer sits.  A controller that is not
one of hedit's (any callable with the reference's signature) is called through the executor's hook on
materialised probabilities (hedit/unet.py::forward_hooked).

The original Prompt-to-Prompt workflow of the same file is here too: init_latent (:190-197), diffusion_step (:166-178),
text2image_ldm_stable (:231-275) -- a source / target pair generated from one noise sample under a controller -- and the
viewers' helpers view_images (:137-162) and text_under_image (:124-134).  The loop is one 4n-row UNet call and one
hedit_step_pair launch per step; text2image_batch is its lock-step form over a ControllerBatch.
"""
import numpy as np
import torch

from .seq_aligner import get_word_inds  # noqa: F401  (re-exported like the reference)


class P2PCrossAttnProcessor:
    def __init__(self, controller, place_in_unet):
        self.controller = controller
        self.place_in_unet = place_in_unet

    def __call__(self, *a, **k):
        raise RuntimeError("the attention body of P2PCrossAttnProcessor is the HIP kernels (fused), or the executor's hook "
                           "path for a host-language controller (hedit.unet.UNet2DConditionModel.forward_hooked); the "
                           "processor object itself is a marker and cannot be called")


def register_attention_control(model, controller):
    procs = {}
    for name in model.unet.attn_processors.keys():
        if name.startswith("mid_block"):
            place = "mid"
        elif name.startswith("up_blocks"):
            place = "up"
        elif name.startswith("down_blocks"):
            place = "down"
        else:
            continue
        procs[name] = P2PCrossAttnProcessor(controller=controller, place_in_unet=place)
    model.unet.set_attn_processor(procs)
    controller.num_att_layers = len(procs)


def update_alpha_time_word(alpha, bounds, prompt_ind, word_inds=None):
    if isinstance(bounds, float):
        bounds = 0, bounds
    start, end = int(bounds[0] * alpha.shape[0]), int(bounds[1] * alpha.shape[0])
    if word_inds is None:
        word_inds = torch.arange(alpha.shape[2])
    alpha[:start, prompt_ind, word_inds] = 0
    alpha[start:end, prompt_ind, word_inds] = 1
    alpha[end:, prompt_ind, word_inds] = 0
    return alpha


def get_time_words_attention_alpha(prompts, num_steps, cross_replace_steps, tokenizer, max_num_words=77):
    if not isinstance(cross_replace_steps, dict):
        cross_replace_steps = {"default_": cross_replace_steps}
    if "default_" not in cross_replace_steps:
        cross_replace_steps["default_"] = (0.0, 1.0)
    n_edit = len(prompts) - 1
    table = torch.zeros(num_steps + 1, n_edit, max_num_words)
    for i in range(n_edit):
        table = update_alpha_time_word(table, cross_replace_steps["default_"], i)
    for word, bounds in cross_replace_steps.items():
        if word == "default_":
            continue
        for i in range(n_edit):
            ind = get_word_inds(prompts[i + 1], word, tokenizer)
            if len(ind) > 0:
                table = update_alpha_time_word(table, bounds, i, torch.as_tensor(ind))
    return table.reshape(num_steps + 1, n_edit, 1, 1, max_num_words)


@torch.no_grad()
def latent2image(vae, latents):
    """latents -> uint8 HWC numpy images (reference ptp_utils.py:181-187): decode(latents / 0.18215),
    (x / 2 + 0.5).clamp(0, 1) * 255."""
    image = vae.decode(1 / 0.18215 * latents)["sample"]
    image = (image / 2 + 0.5).clamp(0, 1)
    return (image.cpu().permute(0, 2, 3, 1).numpy() * 255).astype("uint8")


# ---------------------------------------------------------------------------------------------- viewers
def text_under_image(image, text, text_color=(0, 0, 0)):
    """The image on a white canvas h + int(0.2 h) high with ``text`` centred in the strip below it (reference
    ptp_utils.py:124-134).  The canvas geometry is the reference's; the glyph pixels are not: the reference draws
    OpenCV's Hershey font, this build draws PIL's default font with ImageDraw (cv2 is not a dependency)."""
    from PIL import Image, ImageDraw, ImageFont
    h, w, c = image.shape
    offset = int(h * .2)
    img = np.ones((h + offset, w, c), dtype=np.uint8) * 255
    img[:h] = image
    canvas = Image.fromarray(img)
    draw = ImageDraw.Draw(canvas)
    font = ImageFont.load_default()
    left, top, right, bottom = draw.textbbox((0, 0), text, font=font)
    draw.text(((w - (right - left)) // 2 - left, h + (offset - (bottom - top)) // 2 - top), text, fill=tuple(text_color), font=font)
    return np.array(canvas)


def view_images(images, num_rows=1, offset_ratio=0.02):
    """A list / (N,H,W,3) stack / one HWC uint8 image as one PIL grid of num_rows rows, int(h * offset_ratio) white
    pixels between cells, white filler cells where the count does not divide (reference ptp_utils.py:137-162, whose
    filler count ``len % num_rows`` is kept)."""
    from PIL import Image
    if type(images) is list:
        num_empty = len(images) % num_rows
    elif images.ndim == 4:
        num_empty = images.shape[0] % num_rows
    else:
        images = [images]
        num_empty = 0
    filler = np.ones(images[0].shape, dtype=np.uint8) * 255
    images = [im.astype(np.uint8) for im in images] + [filler] * num_empty
    h, w, _ = images[0].shape
    offset = int(h * offset_ratio)
    num_cols = len(images) // num_rows
    grid = np.ones((h * num_rows + offset * (num_rows - 1), w * num_cols + offset * (num_cols - 1), 3), dtype=np.uint8) * 255
    for i in range(num_rows):
        for j in range(num_cols):
            y, x = i * (h + offset), j * (w + offset)
            grid[y:y + h, x:x + w] = images[i * num_cols + j]
    return Image.fromarray(grid)


# ---------------------------------------------------------------------------------------------- generation
_PAIR_ONLY = ("one (source, target) prompt pair per controller, as in the h-Edit drivers; stack controllers with "
              "ControllerBatch")
_LOW_RESOURCE = ("low_resource (ptp_classes.LOW_RESOURCE): the reference then evaluates the unconditional and the text half "
                 "in two 2-row UNet passes, a plan layout the attention kernels do not have; only the one 4n-row pass is built")


def init_latent(latent, model, height, width, generator, batch_size):
    """(latent, latents) as the reference (ptp_utils.py:190-197): x_T (1,C,h/8,w/8) is drawn on the CPU with the
    caller's generator -- a seed gives the reference's noise -- and expanded to the batch on the model's device."""
    ch = model.unet.config["in_channels"]
    if latent is None:
        latent = torch.randn((1, ch, height // 8, width // 8), generator=generator)
    latents = latent.expand(batch_size, ch, height // 8, width // 8).to(model.device)
    return latent, latents


def _row_guidance(guidance_scale, n):
    """guidance per latent row [src]*n, [tar]*n from a float, one value per prompt of the pair, or one per row"""
    if isinstance(guidance_scale, torch.Tensor):
        guidance_scale = guidance_scale.reshape(-1).tolist()
    if isinstance(guidance_scale, (int, float)):
        return [float(guidance_scale)] * (2 * n)
    g = [float(v) for v in guidance_scale]
    if len(g) == 2:
        return [g[0]] * n + [g[1]] * n
    if len(g) != 2 * n:
        raise ValueError(f"guidance_scale: a float, one value per prompt (2) or one per latent row ({2 * n}) expected, got {len(g)}")
    return g


@torch.no_grad()
def diffusion_step(model, controller, latents, context, t, guidance_scale, low_resource=False):
    """One generation step (reference ptp_utils.py:166-178) for n pairs in lock-step: latents (2n,C,H,W) laid out
    [x_src]*n, [x_tar]*n and context (4n,77,D) = cat([uncond, text]) -- for n = 1 the reference's batch.  One 4n-row
    UNet call under the registered controller ([x_src|null]*n, [x_tar|null]*n, [x_src|src]*n, [x_tar|tar]*n, the
    reference's ``torch.cat([latents] * 2)``), then CFG and the eta = 0 reverse step in ONE hedit_step_pair launch
    (n_kinds = 2: guidance_scale, a float or one value per prompt, is c[k].w_src), then controller.step_callback.
    Guidance that differs between the images of a batch takes one launch per row: the same arithmetic per element.
    Nothing here waits for the device."""
    from ..engine import HEditEngine, Schedule
    from . import ptp_classes
    if low_resource or ptp_classes.LOW_RESOURCE:
        raise NotImplementedError(_LOW_RESOURCE)
    if latents.dim() != 4 or latents.shape[0] % 2:
        raise ValueError("latents: (2n, C, H, W) laid out [x_src]*n, [x_tar]*n expected")
    n = latents.shape[0] // 2
    latents = latents.to(device=model.device, dtype=torch.float32).contiguous()
    e = model.unet(torch.cat([latents] * 2), t, encoder_hidden_states=context)["sample"]
    e_u, e_c = e[:2 * n], e[2 * n:]
    w = _row_guidance(guidance_scale, n)
    S, eng, tt = Schedule(model.scheduler), HEditEngine(model), int(t)

    def coef(weight):
        return S.step_coef(tt, 0, 0.0, False, (weight, 0.0, 0.0), coeff=0.0)
    out = torch.empty_like(latents)
    if len(set(w[:n])) == 1 and len(set(w[n:])) == 1:
        eng.step_pair(e_u, e_c, latents, None, out, n, 2, [coef(w[0]), coef(w[n])])
    else:
        for r in range(2 * n):
            eng.step_pair(e_u[r:r + 1], e_c[r:r + 1], latents[r:r + 1], None, out[r:r + 1], 1, 1, [coef(w[r])])
    return controller.step_callback(out)


def _encode(model, prompts):
    """prompt embeddings through model.text_encoder, whichever encoder that is, with the bits of single-prompt calls
    (hedit.engine.HEditEngine.encode)"""
    from ..engine import HEditEngine
    return HEditEngine(model).encode(prompts)


@torch.no_grad()
def text2image_batch(model, pairs, controller_batch, num_inference_steps=50, guidance_scale=7.5, generators=None, latents=None):
    """Prompt-to-Prompt generation for n [source, target] pairs in lock-step (build-side form of text2image_ldm_stable
    over ptp_controller_utils.make_controller_batch; a single controller serves n = 1).  Rows are [src]*n, [tar]*n; the
    two prompts of a pair share ONE x_T: latents[i] (1,C,h,w) / (C,h,w) where given, else drawn on the CPU with
    generators[i].  guidance_scale: a float, (source, target), or one value per row.
    -> (latents (2n,C,h,w), x_T (n,C,h,w)); image i has the bits of its single-pair call."""
    pairs = [list(p) for p in pairs]
    if not pairs or any(len(p) != 2 for p in pairs):
        raise NotImplementedError(_PAIR_ONLY)
    n = len(pairs)
    members = getattr(controller_batch, "controllers", None)
    if members is not None and len(members) != n:
        raise ValueError(f"{n} prompt pair(s) for a batch of {len(members)} controller(s)")
    if members is None and n != 1:
        raise ValueError("several pairs need a ControllerBatch (ptp_controller_utils.make_controller_batch)")
    register_attention_control(model, controller_batch)
    size = model.unet.config["sample_size"] * 8
    generators = list(generators) if generators is not None else [None] * n
    given = list(latents) if latents is not None else [None] * n
    if len(generators) != n or len(given) != n:
        raise ValueError("one generator / latent per pair expected")
    x_T = []
    for gen, lat in zip(generators, given):
        if lat is not None:
            lat = lat.reshape(1, *lat.shape[-3:])
        hw = (size, size) if lat is None else (lat.shape[-2] * 8, lat.shape[-1] * 8)
        x_T.append(init_latent(lat, model, hw[0], hw[1], gen, 1)[0])
    x_T = torch.cat(x_T)
    x = x_T.to(device=model.device, dtype=torch.float32)
    x = torch.cat([x, x]).contiguous()
    null = _encode(model, [""]).expand(2 * n, -1, -1)
    context = torch.cat([null, _encode(model, [p[0] for p in pairs]), _encode(model, [p[1] for p in pairs])]).contiguous()
    model.scheduler.set_timesteps(num_inference_steps)
    for t in model.scheduler.timesteps:
        x = diffusion_step(model, controller_batch, x, context, t, guidance_scale)
    return x, x_T


@torch.no_grad()
def text2image_ldm_stable(model, prompt, controller, num_inference_steps=50, guidance_scale=7.5, generator=None, latent=None,
                          restored_wt=None, restored_zs=None, low_resource=False):
    """The reference's generation loop (ptp_utils.py:231-275): registers the controller, encodes the prompts, draws x_T
    once for both prompts and runs the scheduler's timesteps through diffusion_step.  -> (latents (2,C,h,w), latent
    (1,C,h,w)); decode with latent2image.  prompt is a [source, target] pair, as everywhere in this build.  The latent
    size is the UNet's sample_size (64: the reference's 512 pixels) unless ``latent`` says otherwise; restored_wt /
    restored_zs are accepted and unused, as in the reference."""
    if low_resource:
        raise NotImplementedError(_LOW_RESOURCE)
    if isinstance(prompt, str) or len(prompt) != 2:
        raise NotImplementedError(_PAIR_ONLY)
    return text2image_batch(model, [list(prompt)], controller, num_inference_steps, guidance_scale,
                            generators=[generator], latents=None if latent is None else [latent])


def text2image_ldm(*args, **kwargs):
    """Not built: the reference's 256-pixel latent-diffusion variant (ptp_utils.py:200-228) runs a BERT text encoder
    and a VQ-VAE this build has no kernels or checkpoints for; text2image_ldm_stable is the Stable Diffusion loop."""
    raise NotImplementedError("text2image_ldm: the 256-pixel BERT / VQ-VAE latent-diffusion variant is not built; "
                              "use text2image_ldm_stable")
