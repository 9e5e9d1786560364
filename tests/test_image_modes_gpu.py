"""Device pre-processing of RGBA, LA, L, P and 1 images (pg_image_preprocess_modes, pg_image_palette through
pghip.image.preprocess and the processor): bit-exact with the reference's host path (PIL BICUBIC in the image's own
mode, convert("RGB"), rescale, normalise, CHW).  np.array_equal everywhere, no tolerance."""
import numpy as np
import pytest
import torch

import image_modes_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


@pytest.fixture
def spy(monkeypatch):
    """Wraps pghip.image.preprocess: the list of image modes of every call that reached the device path."""
    from pghip import image
    real, calls = image.preprocess, []

    def wrapped(images, *a, **k):
        calls.append([getattr(im, "mode", None) for im in images])
        return real(images, *a, **k)
    monkeypatch.setattr(image, "preprocess", wrapped)
    return calls


@pytest.mark.parametrize("H,W,S", R.SHAPES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_preprocess_modes_bit_exact_with_reference_host_path(kind, H, W, S):
    from pghip import image
    im = R.make_image(kind, H, W)
    out = image.preprocess([im], S)
    assert out.shape == (1, 3, S, S) and out.dtype == torch.float32 and out.is_cuda
    assert np.array_equal(out[0].cpu().numpy(), R.reference(im, S))


def test_fixture_rgba_image_bit_exact(tmp_path):
    """The configs[0] fixture image: 444 x 1004 RGBA with a gradient alpha, as the entry point opens it."""
    from PIL import Image
    import main_fixture as MF
    from pghip import image
    im = Image.open(MF.write_image(str(tmp_path / "pic.png")))
    assert im.mode == "RGBA" and im.size == (MF.IMAGE_HW[1], MF.IMAGE_HW[0])
    assert np.array_equal(image.preprocess([im], 224)[0].cpu().numpy(), R.reference(im, 224))


@pytest.mark.parametrize("kind", ["L", "LA", "RGBA"])
@pytest.mark.parametrize("H,W,S", [(37, 51, 224), (224, 224, 224)])
def test_array_inputs_match_the_pil_image(kind, H, W, S):
    """HxW, HxWx2 and HxWx4 uint8 arrays and tensors are read as L, LA and RGBA."""
    from pghip import image
    im = R.make_image(kind, H, W)
    arr = np.asarray(im, dtype=np.uint8)
    assert arr.shape == (H, W) + {"L": (), "LA": (2,), "RGBA": (4,)}[kind]
    want = image.preprocess([im], S)
    assert torch.equal(image.preprocess([arr], S), want)
    assert torch.equal(image.preprocess([torch.from_numpy(arr.copy())], S), want)


def _rgb_args(H, W, S, dev="cuda"):
    from pghip import image
    src = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    vb, vk, vks, vb_host = image._coeffs_dev(H, S, dev)
    hb, hk, hks, _ = image._coeffs_dev(W, S, dev)
    y0 = int(vb_host[0, 0])
    rows = int(vb_host[-1, 0] + vb_host[-1, 1]) - y0
    lut = torch.from_numpy(image.normalise_lut()).to(dev)
    return src, (hb, hk, hks, vb, vk, vks, y0, rows), lut


@pytest.mark.parametrize("H,W,S", [(37, 51, 224), (480, 640, 224)])
def test_modes_entry_point_with_rgb_equals_the_rgb_entry_point(H, W, S):
    from pghip import ops
    src, tables, lut = _rgb_args(H, W, S)
    rows = tables[-1]
    outs = []
    for fn, extra in ((ops.image_preprocess, ()), (ops.image_preprocess_modes, (3, False))):
        tmp = torch.zeros(rows, S, 3, dtype=torch.uint8, device="cuda")
        out = torch.zeros(3, S, S, dtype=torch.float32, device="cuda")
        fn(src, H, W, *extra, S, *tables, lut, tmp, out)
        outs.append((tmp, out))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][1].abs().sum().item() > 0


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


@pytest.mark.parametrize("kind", ["RGBA", "P7"])
def test_processor_takes_the_device_path(spy, kind):
    from processing_paligemma import PaliGemmaProcessor
    im = R.make_image(kind, 37, 51)
    host = PaliGemmaProcessor(_Tok(), 16, 224, device=None)(images=[im], text=["caption en"])
    assert spy == []
    dev = PaliGemmaProcessor(_Tok(), 16, 224, device="cuda")(images=[im], text=["caption en"])
    assert spy == [[im.mode]]
    assert dev["pixel_values"].is_cuda and dev["pixel_values"].dtype == host["pixel_values"].dtype
    assert torch.equal(dev["pixel_values"].cpu(), host["pixel_values"])


def test_processor_keeps_cmyk_on_the_host(spy):
    from PIL import Image
    from processing_paligemma import PaliGemmaProcessor
    cmyk = np.random.default_rng(5).integers(0, 256, (37, 51, 4), dtype=np.uint8)
    im = Image.frombytes("CMYK", (51, 37), cmyk.tobytes())
    assert im.mode == "CMYK"
    host = PaliGemmaProcessor(_Tok(), 16, 224, device=None)(images=[im], text=["caption en"])
    dev = PaliGemmaProcessor(_Tok(), 16, 224, device="cuda")(images=[im], text=["caption en"])
    assert spy == []
    assert torch.equal(dev["pixel_values"].cpu(), host["pixel_values"])


def test_inference_main_preprocesses_its_rgba_input_on_the_device(golden, tmp_path, capsys, spy):
    """BASELINE configs[0] at TINY size (as test_dropin_gpu.py::test_inference_main_end_to_end_matches_reference, in
    process only): the RGBA fixture image goes through pghip.image.preprocess exactly once, and the 12 greedy ids and
    the printed line are still the ones the reference's own inference.main produced (tests/golden/main.npz)."""
    import main_fixture as MF
    from transformers import PreTrainedTokenizerBase
    import inference
    g = golden("main")
    cfg = MF.write_model_dir(str(tmp_path / "model"))
    assert cfg["text_config"]["vocab_size"] == int(g["vocab_size"])
    assert cfg["image_token_index"] == int(g["image_token_index"])
    img = MF.write_image(str(tmp_path / "pic.png"))
    seen = []
    real = PreTrainedTokenizerBase.decode

    def decode(self, token_ids, *a, **k):
        seen.append([int(t) for t in token_ids])
        return real(self, token_ids, *a, **k)
    PreTrainedTokenizerBase.decode = decode
    try:
        inference.main(model_path=str(tmp_path / "model"), prompt=MF.PROMPT, image_file_path=img,
                       max_tokens_to_generate=MF.MAX_TOKENS, do_sample=False)
    finally:
        PreTrainedTokenizerBase.decode = real
    out = capsys.readouterr().out
    assert seen and seen[-1] == g["ids"].tolist(), (seen, g["ids"].tolist())
    assert len(seen[-1]) == 12
    assert str(g["printed"]) in out, (out[-500:], str(g["printed"]))
    assert spy == [["RGBA"]], spy


def test_modes_entry_point_rejections():
    """Every argument set pg_image_preprocess_modes must reject raises PgHipError through the binding, before any
    launch: the output and tmp buffers keep their fill."""
    from pghip import _lib, ops
    H, W, S = 20, 24, 16
    src, (hb, hk, hks, vb, vk, vks, y0, rows), lut = _rgb_args(H, W, S)
    src4 = torch.zeros(H, W, 4, dtype=torch.uint8, device="cuda")
    sq = torch.zeros(S, S, 4, dtype=torch.uint8, device="cuda")
    tmp = torch.full((H, S, 4), 9, dtype=torch.uint8, device="cuda")
    out = torch.full((3, S, S), 7.0, dtype=torch.float32, device="cuda")
    ok = dict(src=src4, H=H, W=W, C=4, alpha=1, S=S, hb=hb, hk=hk, hks=hks, vb=vb, vk=vk, vks=vks, y0=y0, rows=rows,
              lut=lut, tmp=tmp, out=out)
    bad = {
        "C = 0": dict(C=0, alpha=0),
        "C = 5": dict(C=5, alpha=0),
        "alpha with C = 3": dict(src=src, C=3, alpha=1),
        "alpha with C = 1": dict(C=1, alpha=1),
        "no horizontal table, W != S": dict(hb=None, hk=None, hks=0),
        "no vertical table, H != S": dict(vb=None, vk=None, vks=0, y0=0, rows=H),
        "no table at all, sizes differ": dict(hb=None, hk=None, hks=0, vb=None, vk=None, vks=0, y0=0, rows=H),
        "horizontal bounds without taps": dict(hk=None),
        "vertical bounds without taps": dict(vk=None),
        "tmp missing with a horizontal pass": dict(tmp=None),
        "y0 + rows > H": dict(y0=H - rows + 1),
        "rows > H": dict(y0=0, rows=H + 1),
        "negative y0": dict(y0=-1),
        "no rows": dict(rows=0),
        "H = 0": dict(H=0),
        "S = 0": dict(S=0),
        "misaligned RGBA source": dict(src=src4.view(-1)[1:]),
    }
    for name, change in bad.items():
        try:
            ops.image_preprocess_modes(**{**ok, **change})
        except _lib.PgHipError as e:
            assert "pg_image_preprocess_modes" in str(e)
        else:
            pytest.fail(name + ": accepted")
    # null required pointers (the wrapper dereferences its tensors, so these go through the binding itself)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    for null in ("src", "lut", "out"):
        a = {**ok, null: None}
        with pytest.raises(_lib.PgHipError, match="pg_image_preprocess_modes"):
            _lib.call("pg_image_preprocess_modes", p(a["src"]), H, W, 4, 1, S, p(hb), p(hk), hks, p(vb), p(vk), vks, y0,
                      rows, p(a["lut"]), p(tmp), p(a["out"]), s)
    # same size and no tables is fine only for S x S input
    with pytest.raises(_lib.PgHipError):
        ops.image_preprocess_modes(sq, S, S, 4, 0, S, None, None, 0, None, None, 0, 0, S + 1, lut, None, out)
    torch.cuda.synchronize()
    assert (out == 7.0).all().item() and (tmp == 9).all().item()
    # and the accepted forms of the same buffers do launch
    ops.image_preprocess_modes(**ok)
    ops.image_preprocess_modes(sq, S, S, 4, 1, S, None, None, 0, None, None, 0, 0, S, lut, None, out)
    torch.cuda.synchronize()
    assert torch.equal(out, lut[0].expand(3, S, S))


def test_palette_entry_point_rejections():
    from pghip import _lib, image, ops
    H, W, S = 20, 24, 16
    src = torch.zeros(H, W, dtype=torch.uint8, device="cuda")
    xt = torch.from_numpy(image.nearest_index(W, S)).cuda()
    yt = torch.from_numpy(image.nearest_index(H, S)).cuda()
    pal = torch.from_numpy(image.palette_lut([10, 20, 30])).cuda()
    out = torch.full((3, S, S), 7.0, dtype=torch.float32, device="cuda")
    for change in (dict(H=0), dict(W=0), dict(S=0), dict(xtab=None), dict(ytab=None), dict(pal_lut=None)):
        with pytest.raises(_lib.PgHipError, match="pg_image_palette"):
            ops.image_palette(**{**dict(src=src, H=H, W=W, S=S, xtab=xt, ytab=yt, pal_lut=pal, out=out), **change})
    s = torch.cuda.current_stream().cuda_stream
    for a in ((None, out.data_ptr()), (src.data_ptr(), None)):
        with pytest.raises(_lib.PgHipError, match="pg_image_palette"):
            _lib.call("pg_image_palette", a[0], H, W, S, xt.data_ptr(), yt.data_ptr(), pal.data_ptr(), a[1], s)
    torch.cuda.synchronize()
    assert (out == 7.0).all().item()
    ops.image_palette(src, H, W, S, xt, yt, pal, out)
    torch.cuda.synchronize()
    assert torch.equal(out, pal[0].view(3, 1, 1).expand(3, S, S))
