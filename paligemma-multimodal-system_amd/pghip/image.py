"""GPU image pre-processing: the reference's process_images (processing_paligemma.py:38-73) for 8-bit images
of mode RGB, RGBA, LA, L, P and 1 as HIP passes (pg_image_preprocess, pg_image_preprocess_modes, pg_image_palette).

The resize is PIL's ``Image.resize(..., BICUBIC)`` (Pillow 12.2.0, libImaging/Resample.c — a
third-party algorithm the reference calls, not in /root/reference): separable convolution with the
a = -0.5 cubic kernel widened by the downscale factor, double coefficients normalised per output
pixel and rounded to 22-bit fixed point, a horizontal pass over the rows the vertical pass needs
(rounded and clipped to uint8), then the vertical pass.  The coefficient tables below restate
Pillow's precompute_coeffs / normalize_coeffs_8bpc in the same double arithmetic; the kernels do the
integer accumulation.  The rescale+normalise of the reference (uint8 * (1/255.0) in float64 -> float32,
then (x - 0.5) / 0.5 in float32) is a 256-entry table, so the whole pipeline is bit-exact with the
reference's host path (tests/test_host.py, tests/test_kernels_gpu.py, tests/test_image_modes_*.py).

The reference resizes in the image's own mode and converts to RGB afterwards, so each mode follows PIL's rule for it:

- same size (H == W == S), any mode: ``resize`` copies; only ``convert("RGB")`` applies (no premultiply round trip,
  which is lossy).
- RGBA, LA: colour bytes premultiplied by alpha (``t = c*a + 128; ((t >> 8) + t) >> 8``), every channel -- alpha too --
  through the passes above, then un-premultiplied (a in {0, 255}: unchanged, else ``min(255, 255*c // a)``);
  ``convert("RGB")`` drops alpha without compositing.  The kernels fold the premultiply into the first pass's loads and
  the rest into the last pass's epilogue.
- L (and LA): the grey channel is written three times.
- P, 1: PIL forces NEAREST; the source index is the floor of an *accumulated* double (nearest_index), and
  ``convert("RGB")`` is a palette lookup, composed here with the normalise table (palette_lut).

Every other mode (CMYK, YCbCr, I, I;16, F, ...) raises ValueError: the processor keeps those on the host path.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np
import torch

from . import ops

PRECISION_BITS = 32 - 8 - 2
SUPPORTED_MODES = ("RGB", "RGBA", "LA", "L", "P", "1")
_CHANNELS = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4}


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_coeffs(in_size: int, out_size: int):
    """(bounds int32 [out][2] = (first input index, count), fixed-point taps int32 [out][ksize], ksize)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def nearest_index(in_size: int, out_size: int) -> np.ndarray:
    """int32 [out_size]: the source index PIL's NEAREST resize reads for each output index (Geometry.c
    ImagingScaleAffine): the floor of a double that starts at half a step and is *accumulated* step by step -- the
    closed form floor((x + 0.5) * step) rounds differently and picks other columns (e.g. at 640 -> 224)."""
    step = in_size / out_size
    tab = np.empty(out_size, np.int32)
    xo = step * 0.5
    for x in range(out_size):
        tab[x] = int(xo)
        xo += step
    assert tab.min() >= 0 and tab.max() < in_size, (in_size, out_size)
    return tab


def normalise_lut(scale_factor: float = 1 / 255.0, mean: float = 0.5, std: float = 0.5) -> np.ndarray:
    """float32 [256]: the reference's rescale ((u8 * scale) in float64 -> float32) then normalise in float32."""
    x = (np.arange(256, dtype=np.uint8) * scale_factor).astype(np.float32)
    return (x - np.float32(mean)) / np.float32(std)


def palette_lut(im_or_table) -> np.ndarray:
    """float32 [256][3]: ``convert("RGB")`` of a P or 1 image as a table, composed with normalise_lut.  Takes a PIL
    image (P: ``getpalette()``, which reads RGB out of palettes stored as RGBA too and ignores a PNG's transparency
    entry; 1: black and white) or the palette itself (n <= 256 RGB triples, flat or [n][3]).  Entries past the
    palette's length are black, as in PIL."""
    if hasattr(im_or_table, "mode"):
        if im_or_table.mode == "1":
            table = [0, 0, 0, 255, 255, 255]
        elif im_or_table.mode == "P":
            table = im_or_table.getpalette()
        else:
            raise ValueError(f"pghip.image.palette_lut: mode {im_or_table.mode} has no palette")
    else:
        table = im_or_table
    flat = np.asarray(table, dtype=np.uint8).reshape(-1)
    if flat.size % 3 or flat.size > 768:
        raise ValueError("pghip.image.palette_lut: expected at most 256 RGB triples")
    pal = np.zeros(768, np.uint8)
    pal[:flat.size] = flat
    return normalise_lut()[pal.reshape(256, 3)]


_coeff_cache: dict = {}


def _coeffs_dev(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _coeff_cache:
        b, k, ks = resample_coeffs(in_size, out_size)
        _coeff_cache[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), ks, b)
    return _coeff_cache[key]


def _nearest_dev(in_size, out_size, device):
    key = ("nearest", in_size, out_size, str(device))
    if key not in _coeff_cache:
        _coeff_cache[key] = torch.from_numpy(nearest_index(in_size, out_size)).to(device)
    return _coeff_cache[key]


def _as_source(im):
    """(uint8 tensor [H][W][C] or [H][W], channels C or 0 for a palette image, palette table or None)."""
    if isinstance(getattr(im, "mode", None), str):        # a PIL image (a tensor's .mode is a method)
        if im.mode not in SUPPORTED_MODES:
            raise ValueError(f"pghip.image.preprocess: modes {', '.join(SUPPORTED_MODES)} only (got mode {im.mode})")
        if im.mode in ("P", "1"):
            return torch.from_numpy(np.asarray(im).astype(np.uint8)), 0, palette_lut(im)
        arr = torch.from_numpy(np.asarray(im, dtype=np.uint8).copy())
        return (arr.unsqueeze(2) if im.mode == "L" else arr), _CHANNELS[im.mode], None
    if isinstance(im, np.ndarray) and not im.flags.writeable:       # e.g. np.asarray(pil_image): torch wants its own
        im = im.copy()
    arr = torch.as_tensor(im)
    if arr.dtype != torch.uint8 or arr.dim() not in (2, 3) or (arr.dim() == 3 and arr.shape[2] not in (2, 3, 4)):
        raise ValueError("pghip.image.preprocess: expected HxW, HxWx2, HxWx3 or HxWx4 uint8")
    if arr.dim() == 2:
        arr = arr.unsqueeze(2)
    return arr, arr.shape[2], None


def preprocess(images: Sequence, image_size: int, device="cuda") -> torch.Tensor:
    """uint8 images -> float32 [B, 3, S, S] pixel_values on the HIP device, equal to the reference's process_images +
    stack.  PIL images in a mode of SUPPORTED_MODES, or uint8 arrays / tensors shaped HxW (read as L), HxWx2 (LA),
    HxWx3 (RGB) or HxWx4 (RGBA); any other mode raises ValueError."""
    dev = torch.device(device)
    lut = torch.from_numpy(normalise_lut()).to(dev)
    S = int(image_size)
    out = torch.empty(len(images), 3, S, S, dtype=torch.float32, device=dev)
    for i, im in enumerate(images):
        arr, C, pal = _as_source(im)
        src = arr.to(dev).contiguous()
        H, W = src.shape[0], src.shape[1]
        if pal is not None:
            ops.image_palette(src, H, W, S, _nearest_dev(W, S, dev), _nearest_dev(H, S, dev),
                              torch.from_numpy(pal).to(dev), out[i])
            continue
        hb = hk = None
        hks = 0
        rows, y0 = H, 0
        vb, vk, vks, vb_host = _coeffs_dev(H, S, dev)
        need_h, need_v = W != S, H != S
        if need_h:
            hb, hk, hks, _ = _coeffs_dev(W, S, dev)
            if need_v:                      # only the source rows the vertical pass reads (Resample.c)
                y0 = int(vb_host[0, 0])
                rows = int(vb_host[-1, 0] + vb_host[-1, 1]) - y0
        tmp = torch.empty(rows, S, C, dtype=torch.uint8, device=dev) if need_h else None
        tables = (hb, hk, hks, vb if need_v else None, vk if need_v else None, vks if need_v else 0, y0, rows)
        if C == 3:
            ops.image_preprocess(src, H, W, S, *tables, lut, tmp, out[i])
        else:
            # alpha only where PIL premultiplies: a same-size image is copied, its alpha just dropped
            ops.image_preprocess_modes(src, H, W, C, C in (2, 4) and (need_h or need_v), S, *tables, lut, tmp, out[i])
    return out
