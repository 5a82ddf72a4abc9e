"""The training pieces of the reference's dino/utils.py on the HIP path, and DINO's loss.

  trunc_normal_                 dino/utils.py:482-520  the initialiser of cls_token / pos_embed / Linear weights
  MultiCropWrapper              :564-597  one backbone forward per run of equally sized crops, the head on all rows
  get_params_groups, has_batchnorms, cosine_scheduler, clip_gradients, cancel_gradients_last_layer   :102-168, 600-619
  DINOLoss                      upstream DINO's main_dino.py (the reference loads the checkpoints it makes and does not carry it):
                                cross-entropy between the centred, sharpened teacher softmax of the two global crops and the
                                student's log-softmax of every other crop; the centre is a momentum average of the teacher logits
  ema_update                    the teacher's exponential moving average of main_dino.py's training loop
  GaussianBlur, Solarization    dino/utils.py:36-68 for a uint8 (B, H, W, 3) batch on the device, every image with its own draw
  DataAugmentationDINO, dino_augment_params
                                upstream main_dino.py's multi-crop transform for a batch of decoded tiles: every random choice drawn
                                on the host into per-image tables, then 2 + n resamples (utils.pil_resize) and, per crop size,
                                one colour and one blur call (kernels_augment.hip), byte for byte what the Pillow chain gives

The loss, its gradient, the centre and the EMA are kernels_dino.hip / kernels_optim.hip (include/ocm_vit.h); clip_gradients runs the
gradient-norm table operators of the optimizer, one tensor per table. fp32 tensors on one HIP device; there is no CPU or eager
fall-back. Raw-pointer writes (centre, teacher parameters, clipped gradients) raise the tensors' version counters, as optimizer.py
does, so operand caches and engines see them.
"""
import math
import random

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, data, utils
from ..engine import _p, _require_hip, _stream, _ws
from ..optimizer import get_params_groups  # DINO's two parameter groups: one statement, shared with optimizer.py

__all__ = ["trunc_normal_", "MultiCropWrapper", "DINOLoss", "ema_update", "get_params_groups", "has_batchnorms",
           "cosine_scheduler", "clip_gradients", "cancel_gradients_last_layer", "GaussianBlur", "Solarization",
           "DataAugmentationDINO", "dino_augment_params"]


def trunc_normal_(tensor, mean=0., std=1., a=-2., b=2.):
    """Fill `tensor` in place with N(mean, std^2) restricted to the ABSOLUTE interval [a, b]
    by inverse-CDF sampling, as the reference does (so with std=.02 and the default bounds it
    is effectively an untruncated normal)."""
    def cdf(v):
        return 0.5 * (1.0 + math.erf(v / math.sqrt(2.0)))

    lo, hi = cdf((a - mean) / std), cdf((b - mean) / std)
    with torch.no_grad():
        tensor.uniform_(2.0 * lo - 1.0, 2.0 * hi - 1.0).erfinv_()
        tensor.mul_(std * math.sqrt(2.0)).add_(mean).clamp_(min=a, max=b)
    return tensor


class MultiCropWrapper(nn.Module):
    """backbone + head over a list of crops: consecutive crops of one size (their last dimension) go through the backbone as one
    batch, the outputs are concatenated in crop order and the head runs once over all rows. The backbone's own classifier
    attributes (`fc`, `head`) become nn.Identity(); state-dict keys are `backbone.*` and `head.*`."""

    def __init__(self, backbone, head):
        super().__init__()
        backbone.fc, backbone.head = nn.Identity(), nn.Identity()
        self.backbone = backbone
        self.head = head

    def forward(self, x):
        crops = x if isinstance(x, list) else [x]
        outs, start = [], 0
        for end in range(1, len(crops) + 1):
            if end == len(crops) or crops[end].shape[-1] != crops[start].shape[-1]:
                outs.append(self.backbone(torch.cat(crops[start:end])))
                start = end
        return self.head(outs[0] if len(outs) == 1 else torch.cat(outs))


def has_batchnorms(model):
    return any(isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm)) for m in model.modules())


def cosine_scheduler(base_value, final_value, epochs, niter_per_ep, warmup_epochs=0, start_warmup_value=0):
    """One value per iteration: a linear warm-up from start_warmup_value to base_value over warmup_epochs, then half a cosine from
    base_value to final_value."""
    total, warm = epochs * niter_per_ep, warmup_epochs * niter_per_ep
    ramp = np.linspace(start_warmup_value, base_value, warm) if warmup_epochs > 0 else np.array([])
    it = np.arange(total - warm)
    schedule = np.concatenate((ramp, final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * it / len(it)))))
    assert len(schedule) == total
    return schedule


def cancel_gradients_last_layer(epoch, model, freeze_last_layer):
    """Drop the gradients of the head's last layer during the first freeze_last_layer epochs."""
    if epoch >= freeze_last_layer:
        return
    for n, p in model.named_parameters():
        if "last_layer" in n:
            p.grad = None


def _check_f32_hip(t, what, device=None):
    _require_hip(t, what)
    if t.dtype != torch.float32:
        raise TypeError(f"{what} is {t.dtype}: the HIP path takes float32 only")
    if device is not None and t.device != device:
        raise TypeError(f"{what} lives on {t.device}, others on {device}: one device per call")


def _one_tensor_table(param_ptr, grad_ptr, count):
    return np.array([[param_ptr, grad_ptr, 0, 0, count]], dtype=np.int64)


def clip_gradients(model, clip):
    """Per parameter: its gradient's 2-norm, and the gradient scaled by clip / (norm + 1e-6) when that is below 1 (the
    coefficient the norm operator forms is min(that, 1), and a product with 1.0 keeps every bit). Returns the norms as floats, in
    named_parameters() order: one read-back for all of them at the end."""
    lib = _lib.load()
    grads = [p.grad for _, p in model.named_parameters() if p.grad is not None]
    if not grads:
        return []
    dev = grads[0].device
    held = []
    for g in grads:
        _check_f32_hip(g, "a gradient", dev)
        if not g.is_contiguous():
            raise ValueError(f"a gradient of shape {tuple(g.shape)} is not contiguous")
        held.append(_one_tensor_table(0, g.data_ptr(), g.numel()))
    with torch.cuda.device(dev):
        sumsq = torch.empty(len(grads), dtype=torch.float64, device=dev)
        norms = torch.empty(len(grads), dtype=torch.float32, device=dev)
        coefs = torch.empty(len(grads), dtype=torch.float32, device=dev)
        nbytes = max(lib.ocm_grad_norm_workspace_bytes(t.ctypes.data, 1) for t in held)
        ws = _ws(nbytes, dev)
        stream = _stream()
        for i, t in enumerate(held):
            _lib.check(lib.ocm_op_grad_norm(t.ctypes.data, 1, float(clip), _p(sumsq[i]), _p(norms[i]), _p(coefs[i]), _p(ws), nbytes,
                                            stream))
            _lib.check(lib.ocm_op_grad_scale(t.ctypes.data, 1, _p(coefs[i]), stream))
    torch.autograd.graph.increment_version(grads)
    return norms.tolist()


def ema_update(teacher_params, student_params, momentum):
    """teacher = teacher * momentum + student * (1 - momentum) for every pair, as one multi-tensor call (ocm_op_ema_update cuts the
    table into launches). The teacher tensors' versions are raised, so the teacher's engine uploads them again."""
    teacher_params, student_params = list(teacher_params), list(student_params)
    if len(teacher_params) != len(student_params):
        raise ValueError(f"{len(teacher_params)} teacher tensors for {len(student_params)} student tensors")
    if not teacher_params:
        return
    dev = teacher_params[0].device
    rows = []
    for t, s in zip(teacher_params, student_params):
        _check_f32_hip(t, "a teacher parameter", dev)
        _check_f32_hip(s, "a student parameter", dev)
        if t.shape != s.shape or not t.is_contiguous() or not s.is_contiguous():
            raise ValueError(f"teacher {tuple(t.shape)} and student {tuple(s.shape)} must be contiguous and of one shape")
        rows.append((t.data_ptr(), s.data_ptr(), 0, 0, t.numel()))
    table = np.ascontiguousarray(np.array(rows, dtype=np.int64))
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ocm_op_ema_update(table.ctypes.data, len(rows), float(momentum), _stream()))
    torch.autograd.graph.increment_version(teacher_params)


class _DINOLossFn(torch.autograd.Function):
    """loss = ocm_op_dino_loss(student, teacher, centre); backward: ocm_op_dino_loss_backward, one pass over the logits. Kept for
    the backward: the inputs themselves and (V + 2) * B pairs of float64 row statistics."""

    @staticmethod
    def forward(ctx, student, teacher, center, student_temp, teacher_temp, ncrops):
        lib, dev = _lib.load(), student.device
        B, K = teacher.shape[0] // 2, student.shape[1]
        with torch.cuda.device(dev):
            loss = torch.empty((), dtype=torch.float32, device=dev)
            stats = torch.empty(((ncrops + 2) * B, 2), dtype=torch.float64, device=dev)
            nbytes = lib.ocm_dino_loss_workspace_bytes(B, ncrops, K)
            ws = _ws(nbytes, dev)
            _lib.check(lib.ocm_op_dino_loss(_p(student), _p(teacher), _p(center), student_temp, teacher_temp, B, ncrops, K, _p(loss),
                                            _p(stats), _p(ws), nbytes, _stream()))
        ctx.dims = (B, ncrops, K, student_temp, teacher_temp)
        ctx.save_for_backward(student, teacher, center, stats)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        student, teacher, center, stats = ctx.saved_tensors
        B, V, K, ts, tt = ctx.dims
        dev = student.device
        with torch.cuda.device(dev):
            g = grad_loss.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
            ds = torch.empty_like(student)
            _lib.check(_lib.load().ocm_op_dino_loss_backward(_p(g), _p(student), _p(teacher), _p(center), ts, tt, B, V, K, _p(stats),
                                                             _p(ds), _stream()))
        return ds, None, None, None, None, None


class DINOLoss(nn.Module):
    """Upstream DINO's loss module: `center` is a (1, out_dim) buffer of zeros, the teacher temperature of an epoch comes from
    concatenate(linspace(warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs), full(nepochs - warmup_teacher_temp_epochs,
    teacher_temp)). forward(student_output (ncrops * B, out_dim) crop-major, teacher_output (2 * B, out_dim), epoch) returns the
    loss as a 0-dim tensor whose backward is a HIP kernel, then updates the centre from the teacher output under no_grad:
    center = center * m + (sum of the teacher rows over every rank / (rows * world size)) * (1 - m)."""

    def __init__(self, out_dim, ncrops, warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs, nepochs, student_temp=0.1,
                 center_momentum=0.9):
        super().__init__()
        self.student_temp = student_temp
        self.center_momentum = center_momentum
        self.ncrops = ncrops
        self.register_buffer("center", torch.zeros(1, out_dim))
        self.teacher_temp_schedule = np.concatenate((np.linspace(warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs),
                                                     np.ones(nepochs - warmup_teacher_temp_epochs) * teacher_temp))

    def _check(self, student_output, teacher_output):
        _check_f32_hip(student_output, "student_output")
        _check_f32_hip(teacher_output, "teacher_output", student_output.device)
        _check_f32_hip(self.center, "the center buffer", student_output.device)
        K = self.center.shape[1]
        if student_output.dim() != 2 or teacher_output.dim() != 2 or student_output.shape[1] != K or teacher_output.shape[1] != K:
            raise ValueError(f"student_output {tuple(student_output.shape)} and teacher_output {tuple(teacher_output.shape)} must be "
                             f"(rows, {K})")
        if self.ncrops < 2 or teacher_output.shape[0] < 2 or teacher_output.shape[0] % 2 or \
                student_output.shape[0] * 2 != self.ncrops * teacher_output.shape[0]:
            raise ValueError(f"{student_output.shape[0]} student rows and {teacher_output.shape[0]} teacher rows do not make "
                             f"{self.ncrops} crops (at least 2) of a batch and its 2 global crops")

    def forward(self, student_output, teacher_output, epoch):
        self._check(student_output, teacher_output)
        temp = float(self.teacher_temp_schedule[epoch])
        teacher = teacher_output.detach().contiguous()
        # (a copy of the centre: the backward reads the values of this call, and the update below writes the buffer in place)
        loss = _DINOLossFn.apply(student_output.contiguous(), teacher, self.center.detach().reshape(-1).clone(),
                                 float(self.student_temp), temp, int(self.ncrops))
        self.update_center(teacher)
        return loss

    @torch.no_grad()
    def update_center(self, teacher_output):
        lib, dev = _lib.load(), teacher_output.device
        teacher = teacher_output.detach().contiguous()
        rows, K = teacher.shape
        dist = torch.distributed
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        with torch.cuda.device(dev):
            batch_sum = torch.empty(K, dtype=torch.float32, device=dev)
            _lib.check(lib.ocm_op_dino_center(_lib.OCM_DINO_CENTER_SUM, _p(teacher), rows, K, _p(batch_sum), None, 0.0, 0.0,
                                              _stream()))
            if world > 1:
                dist.all_reduce(batch_sum)
            _lib.check(lib.ocm_op_dino_center(_lib.OCM_DINO_CENTER_UPDATE, None, 0, K, _p(batch_sum), _p(self.center),
                                              float(rows * world), float(self.center_momentum), _stream()))
        torch.autograd.graph.increment_version(self.center)


# ---- the multi-crop augmentation (dino/utils.py:36-68; upstream main_dino.py DataAugmentationDINO; kernels_augment.hip) ----------
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SOLARIZE_THRESHOLD, SOLARIZE_OFF = 128, 256  # ImageOps.solarize's default; a threshold no byte reaches


class GaussianBlur:
    """dino/utils.py:36-54 for a batch: per image `random() <= p`, then `uniform(radius_min, radius_max)`, from `rng` (a
    random.Random; the module's global stream when None), and Pillow's ImageFilter.GaussianBlur of that radius on the device. An
    image that is not blurred has radius 0, which copies it: one call serves the batch."""

    def __init__(self, p=0.5, radius_min=0.1, radius_max=2., rng=None):
        self.prob = p
        self.radius_min = radius_min
        self.radius_max = radius_max
        self.rng = rng

    def draw(self):
        """The radius of one image: 0.0 when it is not blurred."""
        rng = self.rng or random
        if not rng.random() <= self.prob:
            return 0.0
        return rng.uniform(self.radius_min, self.radius_max)

    def __call__(self, images_u8):
        return utils.pil_gaussian_blur(images_u8, np.array([self.draw() for _ in range(images_u8.shape[0])], np.float32))


class Solarization:
    """dino/utils.py:57-68 for a batch: per image `random() < p` from `rng`, then ImageOps.solarize on the device."""

    def __init__(self, p, rng=None):
        self.p = p
        self.rng = rng

    def draw(self):
        return (self.rng or random).random() < self.p

    def __call__(self, images_u8):
        on = np.array([self.draw() for _ in range(images_u8.shape[0])], bool)
        return utils.pil_color(images_u8, utils.COLOR_NONE, 0.0, solarize=on, threshold=SOLARIZE_THRESHOLD)


def _color_jitter_params(generator, brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1):
    """torchvision's ColorJitter.get_params on a torch.Generator: randperm(4), then one uniform_ each for brightness, contrast,
    saturation and hue. Returns the four slots in the order they run as (op, factor): the enhancement factor as the float32 Pillow
    receives, for the hue the byte shift int(hue_factor * 255) modulo 256 (the uint8 cast of torchvision's adjust_hue on x86)."""
    order = torch.randperm(4, generator=generator).tolist()
    ranges = ((max(0.0, 1.0 - brightness), 1.0 + brightness), (max(0.0, 1.0 - contrast), 1.0 + contrast),
              (max(0.0, 1.0 - saturation), 1.0 + saturation), (-hue, hue))
    values = [float(torch.empty(1).uniform_(lo, hi, generator=generator)) for lo, hi in ranges]
    values[3] = float(int(values[3] * 255) % 256)
    return [(fn + 1, values[fn]) for fn in order]  # utils.COLOR_BRIGHTNESS .. COLOR_HUE are torchvision's fn_id + 1


def dino_augment_params(batch, height, width, global_crops_scale=(0.4, 1.), local_crops_scale=(0.05, 0.4), local_crops_number=8,
                        generator=None, rng=None):
    """Every random choice of upstream's DataAugmentationDINO for `batch` images of height x width, drawn on the host: image after
    image and, within an image, view after view (global 1, global 2, the local views), each in its Compose's order:
      RandomResizedCrop.get_params (data.random_resized_crop_params), rand(1) < 0.5 for the flip, rand(1) for RandomApply (the
      jitter runs unless 0.8 < it) and only then ColorJitter.get_params (randperm(4) and four uniform_), rand(1) < 0.2 for grey,
      all from `generator` (a torch.Generator; torch's global stream when None); then GaussianBlur's draws (p = 1.0, 0.1, 0.5
      for global 1, global 2, local) and, for global 2, Solarization's (p = 0.2) from `rng` (a random.Random, or the module's).
    Returns one table per view, 2 + local_crops_number dicts of numpy arrays over the images: crops (B,4) int64 (x0, y0, x1, y1),
    hflip (B,) bool, ops (B,4) int32 and factors (B,4) float32 (utils.pil_color's slots; all COLOR_NONE when RandomApply
    skipped the jitter), grey (B,) bool, radius (B,) float32 (0: not blurred), solarize (B,) bool.
    torchvision is not installed here, so the parity of the torch stream with a live torchvision is unpinned, as for
    data.random_resized_crop_params; what the tables do to the pixels is pinned on live Pillow (tests/test_augment_host.py)."""
    B, V = int(batch), 2 + int(local_crops_number)
    blurs = [GaussianBlur(1.0, rng=rng), GaussianBlur(0.1, rng=rng)] + [GaussianBlur(0.5, rng=rng)] * (V - 2)
    solarization = Solarization(0.2, rng=rng)
    views = [dict(crops=np.zeros((B, 4), np.int64), hflip=np.zeros(B, bool), ops=np.zeros((B, 4), np.int32),
                  factors=np.zeros((B, 4), np.float32), grey=np.zeros(B, bool), radius=np.zeros(B, np.float32),
                  solarize=np.zeros(B, bool)) for _ in range(V)]
    for b in range(B):
        for v, view in enumerate(views):
            i, j, h, w = data.random_resized_crop_params(height, width, global_crops_scale if v < 2 else local_crops_scale,
                                                         generator=generator)
            view["crops"][b] = (j, i, j + w, i + h)
            view["hflip"][b] = bool(torch.rand(1, generator=generator).item() < 0.5)
            if not 0.8 < torch.rand(1, generator=generator).item():
                slots = _color_jitter_params(generator)
                view["ops"][b] = [op for op, _ in slots]
                view["factors"][b] = [f for _, f in slots]
            view["grey"][b] = bool(torch.rand(1, generator=generator).item() < 0.2)
            view["radius"][b] = blurs[v].draw()
            if v == 1:
                view["solarize"][b] = solarization.draw()
    return views


class DataAugmentationDINO:
    """Upstream main_dino.py's DataAugmentationDINO for a batch of decoded tiles on the device. __call__ takes uint8 (B, H, W, 3)
    and returns the list MultiCropWrapper takes: 2 + local_crops_number float32 tensors (B, 3, S, S), element v holding view v of
    every image (S = global_size for the first two, local_size after them). The transforms are upstream's: RandomResizedCrop
    (BICUBIC), a flip (0.5), RandomApply(ColorJitter(0.4, 0.4, 0.2, 0.1), 0.8), RandomGrayscale(0.2), GaussianBlur (p = 1.0 / 0.1
    / 0.5), Solarization(0.2) on the second global view, ToTensor and Normalize with ImageNet's mean and std.
    A step is 2 + n resample calls (one per view, every image with its own rectangle and flip) and, per crop size, one colour call
    and one blur call on that size's views concatenated; the blur's column launch solarizes, converts and normalises as it stores."""

    def __init__(self, global_crops_scale=(0.4, 1.), local_crops_scale=(0.05, 0.4), local_crops_number=8, global_size=224,
                 local_size=96, generator=None, rng=None):
        self.global_crops_scale, self.local_crops_scale = tuple(global_crops_scale), tuple(local_crops_scale)
        self.local_crops_number = int(local_crops_number)
        self.global_size, self.local_size = int(global_size), int(local_size)
        self.generator, self.rng = generator, rng
        self.mean, self.std = IMAGENET_MEAN, IMAGENET_STD

    def params(self, batch, height, width):
        return dino_augment_params(batch, height, width, self.global_crops_scale, self.local_crops_scale, self.local_crops_number,
                                   self.generator, self.rng)

    def __call__(self, images_u8, params=None):
        if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
            raise ValueError(f"expected a uint8 (B, H, W, 3) batch of decoded tiles, got {getattr(images_u8, 'dtype', type(images_u8))} "
                             f"{tuple(getattr(images_u8, 'shape', ()))}")
        _require_hip(images_u8, "images")
        B, H, W, _ = images_u8.shape
        views = self.params(B, H, W) if params is None else list(params)
        if len(views) != 2 + self.local_crops_number:
            raise ValueError(f"{len(views)} view tables for 2 + {self.local_crops_number} views")
        out = []
        for group, size in ((views[:2], self.global_size), (views[2:], self.local_size)):
            if not group:
                continue
            crops = torch.cat([utils.pil_resize(images_u8, (size, size), utils.BICUBIC, crop=v["crops"], hflip=v["hflip"],
                                                to_tensor=False) for v in group])
            table = {k: np.concatenate([np.asarray(v[k]) for v in group]) for k in ("ops", "factors", "grey", "radius", "solarize")}
            utils.pil_color(crops, table["ops"], table["factors"], grey=table["grey"], out=crops)
            done = utils.pil_gaussian_blur(crops, table["radius"],
                                           solarize=np.where(table["solarize"], SOLARIZE_THRESHOLD, SOLARIZE_OFF), to_tensor=True,
                                           mean=self.mean, std=self.std)
            out.extend(done[i * B:(i + 1) * B] for i in range(len(group)))
        return out
