"""The attention reference, builders and bound (tests/attn_ref.py) without a device: the CPU emulation of a flash
kernel stays within C / 2 of the fp64 reference on every builder, the builders' own conditions hold (needle weight,
logit range and spike margin are asserted inside them; census counts and bf16 exactness here), and the checks flag an
output computed over one key too few or one stale key too many."""
import math

import numpy as np
import pytest
import torch

import attn_ref as R

DS = (32, 72, 256)
LS = (100, 264, 1000)
NH, NKV = 2, 1


def _inputs(name, D, L, Smax=None, seed=3):
    Smax = Smax or L + 24
    a = (1, NH, NKV, L, D, Smax, [L])
    if name == "census":
        return R.census(*a, seed=seed)
    if name == "needle":
        return R.needle(*a, seed=seed)
    if name == "ramp_up":
        return R.ramp(*a, seed=seed)
    if name == "ramp_down":
        return R.ramp(*a, seed=seed, down=True)
    if name == "spike_last":
        return R.ramp(*a, seed=seed, down=True, spike=[L - 2])
    if name == "spike_mid":
        return R.ramp(*a, seed=seed, down=True, spike=[(L - 1) // 64 * 64 - 64])
    raise ValueError(name)


BUILDERS = ("census", "needle", "ramp_up", "ramp_down", "spike_last", "spike_mid")


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", BUILDERS)
def test_emulation_within_half_the_bound(name, D):
    worst = 0.0
    for L in LS:
        q, k, v = _inputs(name, D, L)
        for t in (q, k, v):
            assert torch.equal(t, R.bf16_exact(t))
        assert torch.equal(v[:, :, L:], torch.full_like(v[:, :, L:], R.POISON_V)) and torch.isfinite(k).all()
        o, budget = R.ref(q, k, v, D ** -0.5, lens=[L])
        for block in (32, 64):
            e = R.emulate(q, k[:, :, :L], v[:, :, :L], D ** -0.5, block)
            if name == "census":
                assert R.census_ok(e, D, [L]), (D, L, block)
            else:
                worst = max(worst, R.worst_ratio(e, o, budget))
    print(f"emulation {name} D={D}: worst |o - ref| / budget = {worst * 256:.3f} * 2^-8")
    assert worst <= R.C / 2, worst


@pytest.mark.parametrize("D", (16, 40, 88))
def test_emulation_within_half_the_bound_at_the_other_head_dims(D):
    """C was measured at head_dims 32, 72 and 256.  test_attn_structured_gpu.test_every_head_dim_instance also runs
    needle and ramp at 16, 40 and 88 (the other (DP, DT) kernel instances) under the same C, at L = 70: the emulation
    stays within C / 2 there too, at that length and over several key blocks."""
    worst = 0.0
    for name in ("needle", "ramp_up", "ramp_down"):
        for L in (70, 264):
            q, k, v = _inputs(name, D, L)
            o, budget = R.ref(q, k, v, D ** -0.5, lens=[L])
            for block in (32, 64):
                e = R.emulate(q, k[:, :, :L], v[:, :, :L], D ** -0.5, block)
                worst = max(worst, R.worst_ratio(e, o, budget))
    print(f"emulation needle / ramp D={D}: worst |o - ref| / budget = {worst * 256:.3f} * 2^-8")
    assert worst <= R.C / 2, worst


def test_the_bound_is_twice_the_measured_worst_rounded_up_to_a_power_of_two():
    assert R.C == 2.0 ** math.ceil(math.log2(2 * R.EMU_WORST))


def test_census_counts_and_reference():
    for D, L in ((32, 1000), (72, 264), (256, 100), (24, 70), (256, 264)):
        q, k, v = R.census(2, 4, 2, 5, D, L + 40, [L, L - 1], seed=1)
        for b, n in enumerate((L, L - 1)):
            cnt = np.bincount(np.arange(n) % D, minlength=D)
            assert np.array_equal(v[b, 0, :n].sum(0).numpy(), cnt)
            assert np.array_equal(R.census_expected(D, n).numpy(), cnt / n)
            assert cnt.max() <= 32
        o, budget = R.ref(q, k, v, D ** -0.5, lens=[L, L - 1])
        assert R.census_ok(o, D, [L, L - 1])
        assert torch.equal(o, budget)
    with pytest.raises(AssertionError):
        R.census(1, 1, 1, 1, 32, 2048, [1025])


@pytest.mark.parametrize("D,L", [(32, 100), (72, 150), (256, 264)])
def test_a_miscounted_key_is_flagged(D, L):
    """One key too few (the last one dropped) and one stale key admitted: census and needle both say so."""
    lens = [L]
    for wrong in ([L - 1], [L + 1]):
        q, k, v = R.census(1, NH, NKV, L, D, L + 24, lens)
        bad, _ = R.ref(q, k, v, D ** -0.5, lens=wrong)
        assert not R.census_ok(bad, D, lens)
        q, k, v = R.needle(1, NH, NKV, L, D, L + 24, lens)
        o, budget = R.ref(q, k, v, D ** -0.5, lens=lens)
        bad, _ = R.ref(q, k, v, D ** -0.5, lens=wrong)
        assert R.within(o, o, budget)
        if wrong[0] < L:                                 # (a stale key of a needle row has next to no weight:
            assert not R.within(bad, o, budget)          # the census, v = +64, is the test of that)


def test_needle_every_key_and_decode_edges():
    D, L = 72, 150
    q, k, v = R.needle(2, 4, 2, L, D, 192, [L, 97], seed=5)
    c = R.needle_gain(D)
    for b, n in enumerate((L, 97)):
        for h in range(4):
            s = (q[b, h, :n] @ k[b, h // 2, :n].t())
            hit = s.argmax(-1)
            assert sorted(hit.tolist()) == list(range(n))          # a permutation: every key is some row's needle
            assert torch.equal(s.max(-1).values, torch.full((n,), c * D))
    edges = [0, 31, 32, 63, 64, L - 2, L - 1, 96, 127, 128]
    fills = R.edge_fills(edges, 3, 1, [L] * 3)
    assert len(fills) == 4 and sorted({f[b][0] for f in fills for b in range(3)}) == sorted(set(edges))
    for f in fills:
        q, k, v = R.needle(3, 4, 1, 1, D, 192, [L] * 3, needles=f)
        for b in range(3):
            assert int((q[b, 0, 0] @ k[b, 0, :L].t()).argmax()) == f[b][0]
    assert R.edge_fills([5, 200], 1, 1, [100]) == [[[5]], [[99]]]


def test_ramp_moves_the_running_max_as_described():
    D, L = 256, 264
    for down in (False, True):
        q, k, v = R.ramp(1, NH, NKV, L, D, L + 24, [L], down=down)
        s = R._logits64(q, k, D ** -0.5, 0, L)
        bm = torch.stack([s[..., i:i + 32].max(-1).values for i in range(0, L, 32)], -1)     # per-block max
        run = torch.cummax(bm, -1).values
        moved = (run[..., 1:] > run[..., :-1])
        assert bool(moved.all()) if not down else not bool(moved.any())
