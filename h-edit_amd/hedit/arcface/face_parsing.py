"""The face-parsing network and the soft face mask of the face-swapping post-processing -- ``FaceParsing`` of the
reference's face-swapping/arcface/face_parsing_model.py (the CelebAMask-HQ U-Net) and ``encode_segmentation`` +
``SoftErosion(13, 0.9, 7)`` of arcface/face_utils.py, as main_edit.py:120-127 / :184-191 use them on the source image.

Both run natively and only natively (csrc/faceparse.hip): ``FaceParsing.forward`` = ``hedit_faceparse_labels``
(split-bf16 precise GEMMs, fp32 activations, argmax fused with the 1x1 classifier), ``face_mask`` = ``hedit_face_mask``.
The torch modules below are PARAMETER CONTAINERS with the reference's state_dict layout (136 entries), so its
``face_parsing.pth`` loads strictly; there is no torch / CPU execution path.

BatchNorm.  The reference never calls ``.eval()`` on this model, so every BatchNorm normalises with the statistics of the
batch it is called with, and it is always called with ONE image.  ``training=True`` (the default, as in the reference)
therefore uses each image's own (mean, biased variance) over H x W: a batch of B images gives exactly the labels of B
separate calls.  This deliberately differs from torch at B > 1, which would pool the statistics over the batch.
``.eval()`` switches to the running statistics."""
import torch
import torch.nn as nn

from ..native import NativeOwner

_FILTERS = (64, 128, 256, 512, 1024)


class _UnetConv2(nn.Module):
    """Parameters of unetConv2 with BatchNorm: (conv3x3 + bias -> BatchNorm2d -> ReLU) x 2"""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1), nn.BatchNorm2d(cout), nn.ReLU())
        self.conv2 = nn.Sequential(nn.Conv2d(cout, cout, 3, 1, 1), nn.BatchNorm2d(cout), nn.ReLU())


class _UnetUp(nn.Module):
    """Parameters of unetUp with is_deconv: ConvTranspose2d(cin, cout, 2, 2) -> cat([skip, up]) -> unetConv2(cin, cout)"""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = _UnetConv2(cin, cout)
        self.up = nn.ConvTranspose2d(cin, cout, kernel_size=2, stride=2)


class FaceParsing(nn.Module, NativeOwner):
    """``FaceParsing()`` of the reference with its default configuration (the only one built).  ``forward(x)``: fp32
    (B, 3, H, W) in [-1, 1] on the GPU, H and W multiples of 16 -> int64 labels (B, 1, H, W) in [0, n_classes).

    The native network is built from the parameters on the first call; ``load_state_dict`` and ``init_random`` drop it,
    other in-place changes of the parameters need ``reset_native()``."""
    _family = "faceparse"
    reset_native = NativeOwner._native_release

    def __init__(self, feature_scale=4, n_classes=19, is_deconv=True, in_channels=3, is_batchnorm=True, device=None):
        super().__init__()
        if feature_scale != 4 or n_classes != 19 or not is_deconv or in_channels != 3 or not is_batchnorm:
            raise NotImplementedError("only the reference's default FaceParsing() is built: feature_scale 4, 19 classes, "
                                      "is_deconv, 3 input channels, is_batchnorm")
        self.feature_scale, self.n_classes, self.is_deconv = feature_scale, n_classes, is_deconv
        self.in_channels, self.is_batchnorm = in_channels, is_batchnorm
        f = [x // feature_scale for x in _FILTERS]
        self.conv1 = _UnetConv2(in_channels, f[0])
        self.maxpool1 = nn.MaxPool2d(kernel_size=2)
        self.conv2 = _UnetConv2(f[0], f[1])
        self.maxpool2 = nn.MaxPool2d(kernel_size=2)
        self.conv3 = _UnetConv2(f[1], f[2])
        self.maxpool3 = nn.MaxPool2d(kernel_size=2)
        self.conv4 = _UnetConv2(f[2], f[3])
        self.maxpool4 = nn.MaxPool2d(kernel_size=2)
        self.center = _UnetConv2(f[3], f[4])
        self.up_concat4 = _UnetUp(f[4], f[3])
        self.up_concat3 = _UnetUp(f[3], f[2])
        self.up_concat2 = _UnetUp(f[2], f[1])
        self.up_concat1 = _UnetUp(f[1], f[0])
        self.final = nn.Conv2d(f[0], n_classes, 1)
        for p in self.parameters():
            p.requires_grad_(False)
        if device is not None:
            self.to(device)

    @property
    def param_shapes(self):
        """{name: shape} of the floating-point state_dict entries (what the native network loads; the integer
        ``num_batches_tracked`` counters are not parameters)"""
        return {k: tuple(v.shape) for k, v in self.state_dict().items() if not k.endswith("num_batches_tracked")}

    def init_random(self, seed=0):
        """seeded synthetic weights (runs without the checkpoint)"""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, t in self.state_dict().items():
                if name.endswith("num_batches_tracked"):
                    continue
                if name.endswith("running_var"):
                    t.copy_(1.0 + 0.2 * torch.rand(t.shape, generator=g))
                elif t.dim() > 1:
                    fan_in = t.shape[0] * t.shape[2] * t.shape[3] if name.endswith("up.weight") else t[0].numel()
                    t.copy_(torch.randn(t.shape, generator=g) * float(fan_in) ** -0.5)
                elif name.endswith("weight"):
                    t.copy_(1.0 + 0.1 * torch.randn(t.shape, generator=g))
                else:
                    t.copy_(0.05 * torch.randn(t.shape, generator=g))
        self.reset_native()
        return self

    def load_state_dict(self, state_dict, strict=True):
        """strict by default like torch; the ``num_batches_tracked`` counters may be absent (they are never read)"""
        sd = {k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
        own = self.state_dict()
        for k, v in own.items():
            if k.endswith("num_batches_tracked"):
                sd[k] = state_dict[k] if isinstance(state_dict.get(k), torch.Tensor) else v
        self.reset_native()
        return super().load_state_dict(sd, strict=strict)

    # ------------------------------------------------------------------ native executor (csrc/faceparse.hip)
    def _native(self, device):
        if self._h is None or self._h_device != device:
            self._native_build(device, self.state_dict())
        return self._h

    @staticmethod
    def _check_shape(x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"FaceParsing takes (B, 3, H, W) images, not {tuple(x.shape)}")
        H, W = x.shape[2], x.shape[3]
        if H < 16 or W < 16 or H % 16 or W % 16:
            raise ValueError(f"FaceParsing needs H and W that are multiples of 16 (the reference's F.pad is then a no-op), "
                             f"got {H} x {W}")

    def forward(self, x):
        from .. import _lib
        self._check_shape(x)
        if not x.is_cuda:
            raise RuntimeError("FaceParsing runs on the HIP executor only: pass a CUDA tensor (there is no CPU / torch path)")
        x = x.detach().float().contiguous()
        B, _, H, W = x.shape
        h = self._native(x.device)
        need = self._lib.hedit_faceparse_workspace_bytes(h, B, H, W)
        if need == 0:
            _lib.check(-1)
        self._grow("_ws", need, x.device)
        labels = torch.empty(B, 1, H, W, dtype=torch.int64, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(self._lib.hedit_faceparse_labels(h, _lib.ptr(x), B, H, W, int(self.training), _lib.ptr(labels),
                                                        _lib.ptr(self._ws), self._ws.numel(), _lib.cur_stream()))
        return labels


def face_mask(labels, kernel_size=13, threshold=0.9, iterations=7):
    """The reference's post-processing mask of parsing labels (main_edit.py:185-191): ``encode_segmentation`` face + mouth
    (the mouth counts twice) through ``SoftErosion(kernel_size, threshold, iterations)``.  labels: int64 (B, 1, H, W) on
    the GPU -> (soft fp32 (B, 1, H, W), hard bool (B, 1, H, W)).

    The maximum that divides the non-hard pixels is taken per image (the reference calls with one image).  Where the
    reference fails we define: no pixel below the threshold -> soft = 1 everywhere; a maximum of 0 (no face pixel
    nearby) -> soft = 0 there instead of 0 / 0."""
    from .. import _lib
    if labels.dim() != 4 or labels.shape[1] != 1 or labels.dtype != torch.int64:
        raise ValueError("face_mask takes int64 labels (B, 1, H, W)")
    if kernel_size < 3 or kernel_size > 31 or kernel_size % 2 == 0 or iterations < 1:
        raise ValueError("face_mask: kernel_size odd in [3, 31] (1 makes SoftErosion's cone 0 / 0), iterations >= 1")
    if not labels.is_cuda:
        raise RuntimeError("face_mask runs on the HIP executor only: pass a CUDA tensor")
    labels = labels.contiguous()
    B, _, H, W = labels.shape
    lib = _lib.lib()
    ws = torch.empty(lib.hedit_face_mask_workspace_bytes(B, H, W), dtype=torch.uint8, device=labels.device)
    soft = torch.empty(B, 1, H, W, dtype=torch.float32, device=labels.device)
    hard = torch.empty(B, 1, H, W, dtype=torch.uint8, device=labels.device)
    with torch.cuda.device(labels.device):
        _lib.check(lib.hedit_face_mask(_lib.ptr(labels), B, H, W, int(kernel_size), float(threshold), int(iterations), _lib.ptr(soft),
                                       _lib.ptr(hard), _lib.ptr(ws), ws.numel(), _lib.cur_stream()))
    return soft, hard.view(torch.bool)
