"""Host half of the device pre-processing of RGBA, LA, L, P and 1 images (pghip/image.py): the numpy restatement
of PIL's per-mode rules (tests/image_modes_ref.py), with the index table and palette the product path uploads
(image.nearest_index, image.palette_lut), equals the reference's host path bit for bit.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import image_modes_ref as R


@pytest.mark.parametrize("H,W,S", R.SHAPES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_mode_restatement_is_bit_exact_with_pil(kind, H, W, S):
    """restatement + nearest_index + palette_lut == Image.resize(BICUBIC).convert("RGB") (+ rescale, normalise, CHW)."""
    from PIL import Image
    from pghip import image
    im = R.make_image(kind, H, W)
    assert im.mode == {"P7": "P", "Prgba": "P"}.get(kind, kind) and im.size == (W, H)
    assert im.mode in image.SUPPORTED_MODES
    rgb = np.array(im.resize((S, S), resample=Image.Resampling.BICUBIC).convert("RGB"))
    if im.mode not in ("P", "1"):
        assert np.array_equal(R.resize_rgb(np.asarray(im, dtype=np.uint8), S), rgb)
    got = R.pixel_values(im, S)
    assert got.dtype == np.float32 and got.shape == (3, S, S)
    assert np.array_equal(got, image.normalise_lut()[rgb].transpose(2, 0, 1))
    assert np.array_equal(got, R.reference(im, S))


def test_alpha_recipe_reaches_the_edge_cases():
    """The alpha planes hold 0, 255 and 1..10 (where min(255, .) clips), and the clip does bite after a resize."""
    rng = np.random.default_rng(0)
    a = R.alpha_plane(rng, 480, 640)
    assert 0.15 < (a == 0).mean() < 0.25 and 0.15 < (a == 255).mean() < 0.25
    assert set(range(1, 11)) <= set(np.unique(a).tolist())
    from oracle.pil_resample import resize_u8
    from pghip.image import resample_coeffs
    pre = resize_u8(R.premultiply(np.asarray(R.make_image("RGBA", 37, 51))), 224, resample_coeffs).astype(np.int64)
    mid = (pre[..., 3:] > 0) & (pre[..., 3:] < 255)
    assert ((255 * pre[..., :3] // np.maximum(pre[..., 3:], 1) > 255) & mid).any()


@pytest.mark.parametrize("n_in,n_out", [(640, 224), (480, 224), (3, 16), (5, 16), (224, 224), (448, 300), (1000, 448)])
def test_nearest_index_is_pils_accumulated_table(n_in, n_out):
    from PIL import Image
    from pghip.image import nearest_index
    tab = nearest_index(n_in, n_out)
    assert tab.dtype == np.int32 and tab.shape == (n_out,) and tab.min() >= 0 and tab.max() < n_in
    ramp = (np.arange(n_in) % 256).astype(np.uint8)
    row = Image.frombytes("P", (n_in, 1), ramp.tobytes()).resize((n_out, 1), resample=Image.Resampling.BICUBIC)
    assert np.array_equal(np.asarray(row)[0], ramp[tab])


def test_nearest_index_differs_from_the_closed_form():
    """floor((x + 0.5) * step) is not what PIL computes: at 640 -> 224 it picks other columns."""
    from pghip.image import nearest_index
    closed = np.floor((np.arange(224) + 0.5) * (640 / 224)).astype(np.int32)
    assert not np.array_equal(nearest_index(640, 224), closed)


def test_palette_lut_tables_and_images():
    from PIL import Image
    from pghip.image import normalise_lut, palette_lut
    lut = normalise_lut()
    short = [1, 2, 3, 250, 251, 252]
    t = palette_lut(short)
    assert t.shape == (256, 3) and t.dtype == np.float32
    assert np.array_equal(t[0], lut[[1, 2, 3]]) and np.array_equal(t[1], lut[[250, 251, 252]])
    assert np.array_equal(t[2:], np.broadcast_to(lut[0], (254, 3)))          # past the palette: black
    assert np.array_equal(palette_lut(np.asarray(short).reshape(2, 3)), t)
    bw = palette_lut(Image.new("1", (2, 2)))
    assert np.array_equal(bw[0], lut[[0, 0, 0]]) and np.array_equal(bw[1], lut[[255, 255, 255]])
    with pytest.raises(ValueError):
        palette_lut(Image.new("RGB", (2, 2)))
    with pytest.raises(ValueError):
        palette_lut([1, 2, 3, 4])


def test_png_transparency_entry_is_ignored(tmp_path):
    """A palette PNG with a tRNS chunk: convert("RGB") ignores it, and so does palette_lut."""
    from PIL import Image
    im = R.make_image("P7", 37, 51)
    path = str(tmp_path / "p.png")
    im.save(path, transparency=3)
    back = Image.open(path)
    assert back.mode == "P" and "transparency" in back.info
    assert np.array_equal(R.pixel_values(back, 224), R.reference(back, 224))


@pytest.mark.parametrize("mode", ["CMYK", "YCbCr", "I", "F", "I;16", "HSV", "LAB"])
def test_other_modes_are_refused_not_converted(mode):
    from PIL import Image
    from pghip import image
    assert mode not in image.SUPPORTED_MODES
    with pytest.raises(ValueError, match="mode"):
        image.preprocess([Image.new(mode, (8, 8))], 16, device="cpu")


def test_bad_arrays_are_refused():
    from pghip import image
    for bad in (np.zeros((4, 4, 5), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4,), np.uint8),
                np.zeros((4, 4, 1), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            image.preprocess([bad], 16, device="cpu")


def test_arrays_and_tensors_are_read_by_shape():
    """HxW, HxWx2, HxWx3, HxWx4 uint8 arrays and tensors -> L, LA, RGB, RGBA sources (a tensor has a .mode too: a method)."""
    from pghip import image
    for shape, C in (((4, 5), 1), ((4, 5, 2), 2), ((4, 5, 3), 3), ((4, 5, 4), 4)):
        a = np.arange(int(np.prod(shape)), dtype=np.uint8).reshape(shape)
        a.flags.writeable = False
        for src in (a, torch.from_numpy(a.copy())):
            arr, c, pal = image._as_source(src)
            assert c == C and pal is None and tuple(arr.shape) == (4, 5, C) and arr.dtype == torch.uint8
            assert np.array_equal(arr.numpy().reshape(shape), a)


class _Tok:
    """The little of a tokenizer PaliGemmaProcessor touches."""
    bos_token = "<bos>"

    def add_special_tokens(self, d):
        pass

    def add_tokens(self, t):
        pass

    def convert_tokens_to_ids(self, t):
        return 7

    def __call__(self, s, **k):
        return {"input_ids": torch.zeros(1, 3, dtype=torch.int64), "attention_mask": torch.ones(1, 3, dtype=torch.int64)}


def test_processor_without_device_keeps_the_host_path_for_rgba(monkeypatch):
    """device=None: an RGBA image's pixel_values are process_images', and pghip.image.preprocess is not called."""
    from processing_paligemma import PaliGemmaProcessor
    from pghip import image
    calls = []
    monkeypatch.setattr(image, "preprocess", lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError))
    im = R.make_image("RGBA", 37, 51)
    out = PaliGemmaProcessor(_Tok(), 16, 224, device=None)(images=[im], text=["caption en"])
    assert not calls
    pv = out["pixel_values"]
    assert pv.dtype == torch.float32 and pv.shape == (1, 3, 224, 224)
    assert np.array_equal(pv[0].numpy(), R.reference(im, 224))
