"""Image pre-processing: the device path (pghip.image.preprocess) against the reference's host path (PIL + numpy +
the H2D copy), for RGBA inputs and for the same images as RGB, so the cost of the alpha work is visible.
    python scripts/tune/image_bench.py [--out FILE]

Per case, after a warm-up (coefficient tables built and cached, code objects loaded), in interleaved rounds:
  host    process_images -> torch.tensor -> .cuda(), host clock around a device synchronise
  device  image.preprocess([im], S) from the PIL image (H2D copy of the uint8 source + the kernels), same clock
  kernels the pg_image_preprocess* launches alone on a resident source, HIP events over REPS back-to-back calls
Median and minimum over the rounds.  Each device result is checked bit-exact against the host result first."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "paligemma-multimodal-system_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402
from pghip import image, ops  # noqa: E402
from processing_paligemma import process_images  # noqa: E402
import main_fixture as MF  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "30"))
REPS = int(os.environ.get("REPS", "200"))
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def fixture_rgba():
    rng = np.random.default_rng(MF.IMAGE_SEED)          # main_fixture.write_image, without the file
    h, w = MF.IMAGE_HW
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    alpha = (np.linspace(40, 255, w)[None, :] * np.ones((h, 1))).astype(np.uint8)
    return Image.fromarray(np.dstack([rgb, alpha]))


def hd_rgba():
    rng = np.random.default_rng(1)
    return Image.fromarray(rng.integers(0, 256, (1080, 1920, 4), dtype=np.uint8))


def host_path(im, S):
    pv = torch.tensor(np.stack(process_images([im], S, scale_factor=1 / 255.0, resampling=Image.Resampling.BICUBIC)))
    pv = pv.cuda()
    torch.cuda.synchronize()
    return pv


def device_path(im, S):
    pv = image.preprocess([im], S)
    torch.cuda.synchronize()
    return pv


def kernel_launcher(im, S, force_modes=False):
    """The launches image.preprocess makes for this image, on buffers that stay resident."""
    dev = "cuda"
    arr = torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).to(dev)
    H, W, C = arr.shape
    vb, vk, vks, vb_host = image._coeffs_dev(H, S, dev)
    hb, hk, hks, _ = image._coeffs_dev(W, S, dev)
    y0 = int(vb_host[0, 0])
    rows = int(vb_host[-1, 0] + vb_host[-1, 1]) - y0
    lut = torch.from_numpy(image.normalise_lut()).to(dev)
    tmp = torch.empty(rows, S, C, dtype=torch.uint8, device=dev)
    out = torch.empty(3, S, S, dtype=torch.float32, device=dev)
    if C == 3 and not force_modes:
        return lambda: ops.image_preprocess(arr, H, W, S, hb, hk, hks, vb, vk, vks, y0, rows, lut, tmp, out), out
    return lambda: ops.image_preprocess_modes(arr, H, W, C, C == 4, S, hb, hk, hks, vb, vk, vks, y0, rows, lut, tmp,
                                              out), out


def clock_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def events_us(run):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS


def fmt(v, unit):
    return f"median {statistics.median(v):9.3f} {unit}  min {min(v):9.3f} {unit}"


assert torch.cuda.is_available(), "image_bench needs the HIP device"
say(f"image pre-processing, {torch.cuda.get_device_name(0)}; {ROUNDS} interleaved rounds, kernels {REPS} calls per round")
for name, rgba, S in (("fixture 444x1004 -> 224", fixture_rgba(), 224), ("1080x1920 -> 448", hd_rgba(), 448)):
    rgb = Image.fromarray(np.asarray(rgba)[..., :3].copy())
    arms = {}
    for mode, im in (("RGBA", rgba), ("RGB", rgb)):
        ref = host_path(im, S)
        assert torch.equal(device_path(im, S), ref), (name, mode)
        arms[f"{mode} host   (PIL + numpy + H2D)"] = (lambda im=im: clock_ms(lambda: host_path(im, S)), "ms")
        arms[f"{mode} device (H2D + kernels)   "] = (lambda im=im: clock_ms(lambda: device_path(im, S)), "ms")
        run, out = kernel_launcher(im, S)
        run()
        torch.cuda.synchronize()
        assert torch.equal(out, ref[0]), (name, mode, "kernels")
        arms[f"{mode} kernels                  "] = (lambda run=run: events_us(run), "us")
    run, out = kernel_launcher(rgb, S, force_modes=True)
    run()
    torch.cuda.synchronize()
    assert torch.equal(out, host_path(rgb, S)[0]), (name, "RGB through the modes entry point")
    arms["RGB kernels, modes entry (C=3) "] = (lambda run=run: events_us(run), "us")
    for fn, _ in arms.values():      # warm-up of every arm
        fn()
    got = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, (fn, _) in arms.items():
            got[k].append(fn())
    say(f"\n{name} (all device results bit-exact with the host path)")
    for k, (_, unit) in arms.items():
        say(f"  {k}  {fmt(got[k], unit)}")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
