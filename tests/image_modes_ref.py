"""numpy restatement of what PIL does to RGBA, LA, L, P and 1 images in the reference's process_images
(``Image.resize(BICUBIC).convert("RGB")``, Pillow 12.2.0), and the images the mode tests run on.

TEST INFRASTRUCTURE ONLY, shared by tests/test_image_modes_host.py (which pins it against PIL itself) and
tests/test_image_modes_gpu.py.  The bicubic passes are oracle/pil_resample.py's; new here are the premultiply /
un-premultiply around them (Convert.c rgbA2rgba / rgba2rgbA), the NEAREST gather and the palette lookup.  The index
table and the palette come from the host half of the product path (pghip.image.nearest_index / palette_lut), as the
coefficient tables do in oracle/pil_resample.py."""
import zlib

import numpy as np

# (H, W, S): tiny upscale, upscale, downscale, horizontal pass only, vertical pass only, same size (a copy in PIL)
SHAPES = [(5, 3, 16), (37, 51, 224), (480, 640, 224), (224, 500, 224), (300, 448, 448), (224, 224, 224)]
# the five modes; P twice: a 7-entry palette, and a palette stored as RGBA -- both with indices past the palette's end
KINDS = ["RGBA", "LA", "L", "P7", "Prgba", "1"]


def premultiply(img: np.ndarray) -> np.ndarray:
    """[H][W][C] uint8, last channel alpha: colour bytes * alpha / 255 rounded as PIL's MULDIV255."""
    a = img[..., -1:].astype(np.int32)
    t = img[..., :-1].astype(np.int32) * a + 128
    out = img.copy()
    out[..., :-1] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out


def unpremultiply(img: np.ndarray) -> np.ndarray:
    """The inverse PIL applies: alpha 0 or 255 leaves the colour, else min(255, 255 * c // a)."""
    a = img[..., -1:].astype(np.int32)
    c = img[..., :-1].astype(np.int32)
    q = np.minimum(255, (255 * c) // np.maximum(a, 1))
    out = img.copy()
    out[..., :-1] = np.where((a == 0) | (a == 255), c, q).astype(np.uint8)
    return out


def to_rgb(img: np.ndarray) -> np.ndarray:
    """convert("RGB") of [H][W][C]: 1 or 2 channels replicate the grey byte, 4 drops alpha without compositing."""
    return np.repeat(img[..., :1], 3, axis=2) if img.shape[2] <= 2 else img[..., :3].copy()


def resize_rgb(img: np.ndarray, S: int) -> np.ndarray:
    """uint8 [H][W] (L) / [H][W][2] (LA) / [H][W][3] / [H][W][4] (RGBA) -> uint8 [S][S][3]."""
    from oracle.pil_resample import resize_u8
    from pghip.image import resample_coeffs
    if img.ndim == 2:
        img = img[..., None]
    H, W, C = img.shape
    if H == S and W == S:               # PIL copies: no premultiply round trip
        return to_rgb(img)
    if C in (2, 4):
        return to_rgb(unpremultiply(resize_u8(premultiply(img), S, resample_coeffs)))
    return to_rgb(resize_u8(img, S, resample_coeffs))


def nearest_gather(idx: np.ndarray, S: int) -> np.ndarray:
    """uint8 [H][W] -> [S][S]: PIL's NEAREST resize (forced for P and 1)."""
    from pghip.image import nearest_index
    H, W = idx.shape
    return idx[nearest_index(H, S)][:, nearest_index(W, S)]


def pixel_values(im, S: int) -> np.ndarray:
    """float32 [3][S][S]: the restatement of process_images([im], S, 1/255.0, BICUBIC)[0] for a PIL image."""
    from pghip.image import normalise_lut, palette_lut
    if im.mode in ("P", "1"):
        hwc = palette_lut(im)[nearest_gather(np.asarray(im).astype(np.uint8), S)]
    else:
        hwc = normalise_lut()[resize_rgb(np.asarray(im, dtype=np.uint8), S)]
    return np.ascontiguousarray(hwc.transpose(2, 0, 1))


def alpha_plane(rng, H: int, W: int) -> np.ndarray:
    """About a fifth of the pixels alpha 0, a fifth 255, the rest uniform in 1..254 (so 1..10 occur, where the clip of
    the un-premultiply bites)."""
    u = rng.random((H, W))
    a = rng.integers(1, 255, (H, W), dtype=np.uint8)
    a[u < 0.2] = 0
    a[u > 0.8] = 255
    return a


def make_image(kind: str, H: int, W: int):
    """The PIL image of one test case, seeded by its kind and size."""
    from PIL import Image
    rng = np.random.default_rng(zlib.crc32(f"{kind}:{H}x{W}".encode()))
    if kind == "RGBA":
        return Image.fromarray(np.dstack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), alpha_plane(rng, H, W)]))
    if kind == "LA":
        return Image.fromarray(np.dstack([rng.integers(0, 256, (H, W), dtype=np.uint8), alpha_plane(rng, H, W)]))
    if kind == "L":
        return Image.fromarray(rng.integers(0, 256, (H, W), dtype=np.uint8))
    if kind == "1":
        return Image.fromarray(rng.random((H, W)) < 0.5)
    im = Image.frombytes("P", (W, H), rng.integers(0, 256, (H, W), dtype=np.uint8).tobytes())   # indices 0..255: past
    #                                                                                             both palettes' ends
    if kind == "P7":
        im.putpalette(rng.integers(0, 256, 7 * 3, dtype=np.uint8).tobytes())
    else:
        assert kind == "Prgba", kind
        im.putpalette(rng.integers(0, 256, 100 * 4, dtype=np.uint8).tobytes(), "RGBA")
    return im


def reference(im, S: int) -> np.ndarray:
    """The reference host path itself (the drop-in's process_images is the reference's, PIL + numpy)."""
    from PIL import Image
    from processing_paligemma import process_images
    return process_images([im], S, scale_factor=1 / 255.0, resampling=Image.Resampling.BICUBIC)[0]
