"""Constrained decoding on the device: pg_dfa_mask, pg_dfa_advance and generate(..., grammar=...).

Everything here is exact.  The two kernels are compared with tests/grammar_ref.py bit for bit (the logits viewed as
int32: NaN payloads, -inf and the padding columns must survive), and a constrained generate must give, id for id, what
grammar_ref.host_loop gives: the same prefill and decode steps without the feature, the mask applied in torch, the
project's own sampler on the masked rows, the DFA stepped in Python.  The project's decode is bit-reproducible and
the mask is defined bitwise, so there is no tolerance to choose.  The only bound is the issue's 1e-5 on the sum of a
top-p distribution."""
import ctypes

import numpy as np
import pytest
import torch

import grammar_ref as GR
import ragged_ref as R

pytestmark = pytest.mark.gpu

NEW = 12
EOS = 1
GUARD_F = np.float32(-1234.5)       # around the logits
SENT_F = np.float32(777.25)         # the padding columns [V, ld)
NAN_A = np.uint32(0x7FC12345).view(np.int32)        # two NaNs with payloads, one of them negative
NAN_B = np.uint32(0xFFC00001).view(np.int32)
NINF = np.float32(-np.inf).view(np.int32)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the HIP device")
    from pghip import _lib
    _lib.load()


def _t(a):
    return torch.from_numpy(np.asarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ tables
def _per(V, unit):
    return ((V + 63) // 64 + unit - 1) // unit * unit


def boundary_tokens(V):
    """0, V - 1 and both sides of every chunk boundary: a row is split over 64 workgroups in chunks of ceil(V / 64)
    tokens rounded up to 8 (csrc/grammar.hip; 4, the argmax kernels' unit, is covered too)."""
    out = {0, V - 1}
    for unit in (8, 4):
        per = _per(V, unit)
        out |= {t for k in range(1, 64) for t in (k * per - 1, k * per) if 0 < k * per < V}
    return sorted(out)


def cases_c2(V, rng):
    """C = 2 (one live class), S = 3: states 0 and 1 allow class 1, state 2 allows nothing.  Three class maps: exactly
    one live token; everything live except a tenth (class 0); the boundary tokens live."""
    trans = np.array([[-1, 1], [-1, 2], [-1, -1]], dtype=np.int16)
    one = np.zeros(V, dtype=np.int16)
    one[int(rng.integers(1, V - 1))] = 1
    most = (rng.random(V) >= 0.1).astype(np.int16)
    bound = np.zeros(V, dtype=np.int16)
    bound[boundary_tokens(V)] = 1
    states = [0, -1, 3, 2, 1, -7, 1000, 0]
    return [(c, trans, states) for c in (one, most, bound)]


def case_big(V, rng):
    """(S, C) = (600, 4096).  Class 1: one token; class 2: the boundary tokens; a twentieth of the rest class 0; the
    others random in [3, C).  State 10 allows class 1 only (exactly one token), 11 everything except class 0, 12 class 2
    only, the rest a random half of the classes; 599 is the last row of trans."""
    S, C = 600, 4096
    cls = rng.integers(3, C, size=V).astype(np.int16)
    cls[rng.random(V) < 0.05] = 0
    cls[boundary_tokens(V)] = 2
    mid = [t for t in range(1, V - 1) if cls[t] != 2]
    cls[mid[len(mid) // 2]] = 1
    live = rng.random((S, C)) < 0.5
    live[10], live[11], live[12] = False, True, False
    live[10, 1] = live[12, 2] = True
    live[:, 0] = False
    trans = np.where(live, rng.integers(0, S, size=(S, C)), -1).astype(np.int16)
    return [(cls, trans, [10, -1, 11, S, 12, 599, 37, S + 3])]


_TABLES = {}


def tables(V):
    if V not in _TABLES:
        rng = np.random.default_rng(V)
        _TABLES[V] = cases_c2(V, rng) + case_big(V, rng)
    return _TABLES[V]


def _dev_i16(a, off=0):
    """a on the device, `off` elements into its allocation (off = 1: not 16-byte aligned, the scalar class loads)."""
    buf = torch.zeros(a.size + off + 8, dtype=torch.int16, device="cuda")
    buf[off:off + a.size] = torch.from_numpy(a).cuda()
    return buf[off:off + a.size]


# ------------------------------------------------------------------------------------------------ pg_dfa_mask
def run_mask(B, V, ld, cls, trans, states, rng, off=4, cls_off=0):
    """One ops.dfa_mask call on [B][V] logits of row stride ld, `off` floats into a guarded allocation; compares the
    whole allocation with grammar_ref.mask_ref bit for bit."""
    from pghip import ops
    S = trans.shape[0]
    n = off + B * ld + 4
    flat = (rng.standard_normal(n) * 3).astype(np.float32)
    flat[:off] = GUARD_F
    flat[off + B * ld:] = GUARD_F
    body = flat[off:off + B * ld].reshape(B, ld)
    body[:, V:] = SENT_F
    bits = body.view(np.int32)
    for b, s in enumerate(states):                 # NaNs and -inf anywhere, and in allowed positions in particular
        where = rng.integers(0, V, size=6).tolist()
        if 0 <= s < S:
            ok = np.nonzero(trans[s][cls] >= 0)[0]
            if ok.size:
                where += rng.choice(ok, size=min(3, ok.size), replace=False).tolist()
        for j, t in enumerate(where):
            bits[b, t] = (NAN_A, NAN_B, NINF)[j % 3]
    want = flat.copy()
    wb = want[off:off + B * ld].reshape(B, ld)
    wb[:] = GR.mask_ref(body, cls, trans, np.asarray(states))
    assert np.array_equal(wb[:, V:].view(np.int32), body[:, V:].view(np.int32))
    dev = torch.from_numpy(flat).cuda()
    view = dev[off:off + B * ld].view(B, ld)[:, :V]
    st = Guarded(states)
    ops.dfa_mask(view, _dev_i16(cls, cls_off), _dev_i16(trans.reshape(-1)).view(trans.shape), st.t)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert st.intact() and st.t.cpu().tolist() == list(states)
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    assert bad.size == 0, (B, V, ld, off, states, bad[:8] - off, got[bad[:8]], want[bad[:8]])
    return got[off:off + B * ld].reshape(B, ld)


class Guarded:
    """int32 words on the device between two guard runs, in one allocation."""

    def __init__(self, init, sentinel=-99, pad=16):
        init = torch.as_tensor(init, dtype=torch.int32).reshape(-1)
        self.n, self.pad, self.sentinel = init.numel(), pad, sentinel
        self.buf = torch.full((self.n + 2 * pad,), sentinel, dtype=torch.int32, device="cuda")
        self.t = self.buf[pad:pad + self.n]
        self.t.copy_(init)

    def intact(self):
        g = torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]]).cpu()
        return bool((g == self.sentinel).all())


def _groups(states, B):
    """`states` as calls of B rows each, the last one filled up from the front."""
    out = []
    for i in range(0, len(states), B):
        g = states[i:i + B]
        out.append((g + states * B)[:B] if len(g) < B else g)
    return out if B <= len(states) else [(states * B)[:B]]


SHAPES = [(1, 300, 300), (3, 1003, 1007), (17, 1174, 1176), (2, 257216, 257216)]


@pytest.mark.parametrize("B,V,ld", SHAPES)
def test_dfa_mask_bit_for_bit(B, V, ld):
    """pg_dfa_mask against mask_ref at (1, 300, 300), (3, 1003, 1007) (an odd stride: only every fourth row can take
    16-byte stores), (17, 1174, 1176) and (2, 257216, 257216), on the C = 2 tables and the (600, 4096) one, with every
    kind of state: free, >= S, exactly one allowed token, everything but class 0, nothing, and the chunk-boundary
    tokens.  The small shapes also run with the logits one float into the allocation (no 16-byte stores at all) and
    with cls two bytes off (scalar class loads)."""
    rng = np.random.default_rng(B * 1000 + V)
    for cls, trans, states in tables(V):
        for g in _groups(states, B):
            run_mask(B, V, ld, cls, trans, g, rng)
    if V < 5000:
        cls, trans, states = tables(V)[-1]
        for off, cls_off in ((1, 0), (4, 1), (3, 3)):
            run_mask(B, V, ld, cls, trans, _groups(states, B)[0], rng, off=off, cls_off=cls_off)


def test_dfa_mask_kinds_do_what_they_say():
    """The state kinds of the tables, spelt out once at (17, 1174, 1176): the one-token state leaves one finite logit,
    the all-but-class-0 state kills exactly the class-0 tokens, the boundary state keeps exactly the boundary tokens,
    and free rows come back untouched (run_mask has already compared every bit)."""
    B, V, ld = 17, 1174, 1176
    rng = np.random.default_rng(5)
    cls, trans, _ = tables(V)[-1]
    states = [10, 11, 12, -1, 600] + [37] * 12
    got = run_mask(B, V, ld, cls, trans, states, rng)[:, :V]
    dead = np.isneginf(got)
    assert (~dead[0]).sum() <= 1 and set(np.nonzero(~dead[0])[0].tolist()) <= set(np.nonzero(cls == 1)[0].tolist())
    assert set(np.nonzero(cls == 0)[0].tolist()) <= set(np.nonzero(dead[1])[0].tolist())
    assert dead[1].sum() <= (cls == 0).sum() + 9                  # (+ the planted -inf words)
    assert set(np.nonzero(~dead[2])[0].tolist()) <= set(boundary_tokens(V))
    assert dead[3].sum() <= 9 and dead[4].sum() <= 9


# ------------------------------------------------------------------------------------------------ pg_dfa_advance
@pytest.mark.parametrize("B,V", [(1, 300), (3, 1003), (17, 1174), (1024, 1174), (5, 257216)])
def test_dfa_advance(B, V):
    """Allowed tokens move the state as advance_ref says and leave err clear, free rows (negative, >= S) stay; then a
    dead token, an id >= V and a negative id keep their rows' states and set err."""
    from pghip import ops
    rng = np.random.default_rng(B + V)
    for cls, trans, _ in (tables(V)[1], tables(V)[-1]):
        S = trans.shape[0]
        cls_d, trans_d = _dev_i16(cls), _dev_i16(trans.reshape(-1)).view(trans.shape)
        usable = np.nonzero((trans[:, np.unique(cls)] >= 0).any(axis=1))[0]     # states that allow some token
        states = rng.choice(usable, size=B).astype(np.int32)
        states[rng.random(B) < 0.25] = -1
        if B > 2:
            states[1], states[2] = S, -5
        ids = np.zeros(B, dtype=np.int64)
        for b, s in enumerate(states.tolist()):
            ok = np.nonzero(trans[s][cls] >= 0)[0] if 0 <= s < S else np.arange(V)
            ids[b] = int(rng.choice(ok))
        want, err = GR.advance_ref(states, ids, cls, trans)
        assert err == 0
        st, er = Guarded(states), Guarded([0])
        ops.dfa_advance(st.t, _t(ids), cls_d, trans_d, er.t)
        torch.cuda.synchronize()
        assert st.intact() and er.intact()
        assert st.t.cpu().tolist() == want.tolist() and int(er.t) == 0
        # one bad row at a time: a dead token, an id >= V, a negative id
        con = [b for b, s in enumerate(states.tolist()) if 0 <= s < S]
        if not con:
            continue
        b = con[0]
        deads = np.nonzero(trans[states[b]][cls] < 0)[0]
        for bad in ([int(deads[0])] if deads.size else []) + [V, V + 12345, -1]:
            ids2 = ids.copy()
            ids2[b] = bad
            want2, err2 = GR.advance_ref(states, ids2, cls, trans)
            assert err2 == 1 and want2[b] == states[b]
            st, er = Guarded(states), Guarded([0])
            ops.dfa_advance(st.t, _t(ids2), cls_d, trans_d, er.t)
            torch.cuda.synchronize()
            assert st.intact() and er.intact()
            assert st.t.cpu().tolist() == want2.tolist() and int(er.t) == 1, bad
        # free rows alone never set err, whatever their ids
        free = np.where(np.arange(B) % 2 == 0, -1, S + np.arange(B)).astype(np.int32)
        st, er = Guarded(free), Guarded([0])
        ops.dfa_advance(st.t, _t(np.full(B, V + 5, dtype=np.int64)), cls_d, trans_d, er.t)
        torch.cuda.synchronize()
        assert st.t.cpu().tolist() == free.tolist() and int(er.t) == 0 and st.intact() and er.intact()


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections_before_any_launch():
    """Null pointers, B outside [1, 1024], V < 1, ld < V with B > 1, S outside [1, 32767] and C outside [2, 4096] are
    refused through the ctypes binding, and the sentinel-filled outputs stay as they were."""
    from pghip import _lib
    B, V, ld, S, C = 2, 64, 64, 3, 2
    logits = torch.full((B * ld,), 5.5, dtype=torch.float32, device="cuda")
    cls = torch.ones(V, dtype=torch.int16, device="cuda")
    trans = torch.full((S * C,), -1, dtype=torch.int16, device="cuda")
    state = torch.zeros(B, dtype=torch.int32, device="cuda")
    ids = torch.zeros(B, dtype=torch.int64, device="cuda")
    err = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def mask(**kw):
        a = dict(logits=p(logits), ld=ld, B=B, V=V, cls=p(cls), trans=p(trans), S=S, C=C, state=p(state))
        a.update(kw)
        _lib.call("pg_dfa_mask", a["logits"], a["ld"], a["B"], a["V"], a["cls"], a["trans"], a["S"], a["C"], a["state"],
                  stream)

    def advance(**kw):
        a = dict(state=p(state), ids=p(ids), B=B, V=V, cls=p(cls), trans=p(trans), S=S, C=C, err=p(err))
        a.update(kw)
        _lib.call("pg_dfa_advance", a["state"], a["ids"], a["B"], a["V"], a["cls"], a["trans"], a["S"], a["C"], a["err"],
                  stream)

    common = [dict(cls=None), dict(trans=None), dict(state=None), dict(B=0), dict(B=-1), dict(B=1025), dict(V=0),
              dict(V=-3), dict(S=0), dict(S=32768), dict(C=1), dict(C=0), dict(C=4097)]
    for kw in common + [dict(logits=None), dict(ld=V - 1), dict(ld=0)]:
        with pytest.raises(_lib.PgHipError, match="pg_dfa_mask"):
            mask(**kw)
    for kw in common + [dict(ids=None), dict(err=None)]:
        with pytest.raises(_lib.PgHipError, match="pg_dfa_advance"):
            advance(**kw)
    torch.cuda.synchronize()
    assert bool((logits == 5.5).all()) and int(err) == -7 and bool((state == 0).all())
    mask(B=1, ld=V - 1)                            # one row: ld is not read
    mask()                                         # ... and the accepted call does run: state 0 allows nothing
    advance()                                      # token 0 is dead in state 0
    torch.cuda.synchronize()
    assert bool(torch.isneginf(logits).all()) and int(err) == 1 and bool((state == 0).all())


# ------------------------------------------------------------------------------------------------ engine (TINY)
@pytest.fixture(scope="module")
def tiny():
    from pghip import configs, engine, synthetic, weights
    cfg = configs.TINY
    return engine.PaliGemmaEngine(cfg, weights.PackedWeights(cfg, synthetic.SyntheticStateDict(cfg).__getitem__))


K_STATES, PER_STATE = 4, 7


def cycle_grammar(V=300, seed=3):
    """An abstract grammar over TINY's 300 ids: K_STATES states in a ring, state s allows its own PER_STATE ids (one
    class) and moves on to state s + 1.  The ids avoid pad / eos / bos and the image token."""
    from pghip.grammar import TokenDFA
    pool = np.random.default_rng(seed).permutation(np.arange(3, V - 1))
    cls = np.zeros(V, dtype=np.int16)
    trans = np.full((K_STATES, K_STATES + 1), -1, dtype=np.int16)
    for s in range(K_STATES):
        cls[pool[s * PER_STATE:(s + 1) * PER_STATE]] = s + 1
        trans[s, s + 1] = (s + 1) % K_STATES
    return TokenDFA(cls, trans, starts=(0,))


BATCHES = [([0], [0]), ([0, 3, 6], [0, -1, 2])]      # (pool requests, start states): B = 1; ragged B = 3, one row free

_SHARED = {}


def shared(tiny, key):
    """What several tests need of a batch, computed once: its inputs, the host loop's ids and the unconstrained ids."""
    if key not in _SHARED:
        rows, starts = BATCHES[key]
        ids, mask, px, _ = R.batch(len(rows), rows=rows)
        inp = (_t(ids), _t(px), _t(mask))
        dfa = cycle_grammar()
        want, seen = GR.host_loop(tiny, inp, dfa, starts, NEW)
        free = tiny.generate(inp[0], inp[1], inp[2], NEW, stop_token=None).tolist()
        _SHARED[key] = SimpleNS(inp=inp, dfa=dfa, starts=starts, want=want, seen=seen, free=free)
    return _SHARED[key]


class SimpleNS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("key", [0, 1])
@pytest.mark.parametrize("use_graph", [True, False])
def test_constrained_greedy_equals_the_host_loop(tiny, key, use_graph):
    """generate(grammar=...) gives exactly grammar_ref.host_loop's ids, graph-replayed and eager (a graph loop that
    starts one DFA transition ahead would allow the wrong ring state's ids from its first step), at B = 1 and on a
    ragged B = 3 batch with three different start states, one of them free; the free row generates what it generates
    without a grammar.  Precondition: every constrained row follows the grammar and the unconstrained run of the same
    prompts does not -- if it ever does, change cycle_grammar's seed, a test input."""
    s = shared(tiny, key)
    B = len(s.starts)
    start = s.starts[0] if B == 1 else s.starts
    got = tiny.generate(*s.inp, NEW, stop_token=None, use_graph=use_graph, grammar=s.dfa, grammar_start=start).tolist()
    for b, st in enumerate(s.starts):
        if st < 0:
            assert got[b] == s.free[b]
            continue
        assert s.dfa.accepts(s.want[b], start=st, prefix=True) and len(set(s.want[b])) > 1
        assert not s.dfa.accepts(s.free[b], start=st, prefix=True), "precondition: change cycle_grammar's seed"
    assert got == s.want, (got, s.want)


def test_grammar_start_defaults_to_the_single_start_state(tiny):
    s = shared(tiny, 0)
    got = tiny.generate(*s.inp, NEW, stop_token=None, grammar=s.dfa).tolist()
    assert got == s.want


def test_constrained_top_p_equals_the_host_loop(tiny):
    """Top-p with explicit uniforms on the ragged batch: the ids equal host_loop's (the same sampler kernel sees the same
    masked bits), graph-replayed and eager, and every constrained id is allowed in the state it was drawn in."""
    s = shared(tiny, 1)
    B = len(s.starts)
    u = torch.rand(NEW + 1, B, generator=torch.Generator().manual_seed(11))
    smp = dict(temperature=0.8, top_p=0.9, uniforms=u)
    want, seen = GR.host_loop(tiny, s.inp, s.dfa, s.starts, NEW, sampler=smp)
    for t in range(NEW):
        for b in range(B):
            assert s.dfa.allowed(seen[t][b])[want[b][t]], (t, b)
    assert want != s.want                                       # the draw is not the greedy pick throughout
    for use_graph in (True, False):
        got = tiny.generate(*s.inp, NEW, do_sample=True, temperature=0.8, top_p=0.9, uniforms=u, stop_token=None,
                            use_graph=use_graph, grammar=s.dfa, grammar_start=s.starts).tolist()
        assert got == want, (use_graph, got, want)


def test_top_p_gives_dead_tokens_no_probability():
    """One ops.topp_sample call on rows pg_dfa_mask has masked: zero probability on every dead token, a sum of 1 within
    1e-5 (the issue's bound), and the drawn id allowed."""
    from pghip import ops
    dfa = cycle_grammar()
    V = dfa.vocab
    x = (torch.randn(3, V, generator=torch.Generator().manual_seed(2)) * 2).cuda()
    states = [1, -1, 3]
    ops.dfa_mask(x, _t(dfa.cls), _t(dfa.trans), _t(np.asarray(states, dtype=np.int32)))
    for top_p in (0.9, 0.3):
        probs = torch.full((3, V), -1.0, device="cuda")
        out = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        u = torch.tensor([[0.5, 0.25, 0.999]], device="cuda")
        ops.topp_sample(x, out, u, temperature=0.8, top_p=top_p, probs_out=probs)
        torch.cuda.synchronize()
        p = probs.cpu().numpy()
        for b, s in enumerate(states):
            ok = dfa.allowed(s)
            assert not p[b][~ok].any() and bool((p[b] >= 0).all()), b
            assert abs(float(p[b].astype(np.float64).sum()) - 1.0) <= 1e-5, (b, p[b].sum())
            assert ok[int(out[b])] and p[b][int(out[b])] > 0


def test_choices(tiny, monkeypatch):
    """from_choices([[5, 6], [5, 7, 8]]): at B = 1 the result is one of the two choices followed by eos and the loop
    stops there (no decode step after the eos); at B = 2 each row ends at its own eos."""
    from pghip.grammar import TokenDFA
    dfa = TokenDFA.from_choices([[5, 6], [5, 7, 8]], EOS, tiny.w.vocab)
    legal = ([5, 6, EOS], [5, 7, 8, EOS])
    ids, mask, px, _ = R.batch(1, rows=[0])
    steps = []
    real = tiny.decode_step
    monkeypatch.setattr(tiny, "decode_step", lambda *a, **k: (steps.append(1), real(*a, **k))[1])
    out = tiny.generate(_t(ids), _t(px), _t(mask), NEW, stop_token=EOS, use_graph=False, grammar=dfa)
    assert out.shape[0] == 1 and out[0].tolist() in legal
    assert len(steps) == out.shape[1] - 1                       # the first token comes from the prefill
    monkeypatch.undo()
    assert tiny.generate(_t(ids), _t(px), _t(mask), NEW, stop_token=EOS, grammar=dfa).tolist() == out.tolist()
    ids, mask, px, _ = R.batch(2, rows=[0, 3])
    rows = tiny.generate(_t(ids), _t(px), _t(mask), NEW, stop_token=EOS, grammar=dfa, return_list=True)
    assert len(rows) == 2 and all(r in legal for r in rows), rows
    padded = tiny.generate(_t(ids), _t(px), _t(mask), NEW, stop_token=EOS, grammar=dfa, pad_token=0)
    for b, r in enumerate(rows):
        assert padded[b, :len(r)].tolist() == r and not padded[b, len(r):].any()


def test_argument_errors_launch_nothing(tiny, monkeypatch):
    from pghip.grammar import TokenDFA
    def never(*a, **k):
        raise AssertionError("the decode state was built")
    monkeypatch.setattr(tiny, "decode_state", never)
    monkeypatch.setattr(tiny, "prefill_request", never)
    ids, mask, px, _ = R.batch(2, rows=[0, 3])
    dfa = cycle_grammar()
    args = (_t(ids), _t(px), _t(mask), NEW)
    for kw in (dict(grammar=cycle_grammar(V=299)), dict(grammar=dfa, grammar_start=K_STATES),
               dict(grammar=dfa, grammar_start=[0, -2]), dict(grammar=dfa, grammar_start=[0]),
               dict(grammar=dfa, grammar_start=[0, 1, 2]), dict(grammar=TokenDFA.union([dfa, dfa]))):
        with pytest.raises(ValueError):
            tiny.generate(*args, **kw)


def test_cli_detect_and_choices_end_to_end(tmp_path, capsys):
    """inference.main with --detect and --choices on the TINY checkpoint directory and the offline tokenizer
    (tests/main_fixture.py): the prompt becomes `detect cat ; dog`, the generated ids follow the detect grammar (TINY's
    300-id vocabulary ends inside the <loc> range: the ids below it are the ones it can emit), and what is printed
    after the answer is the parsed boxes, or why there are none; --choices answers with exactly one choice."""
    import re
    import main_fixture as MF
    from transformers import AutoTokenizer, PreTrainedTokenizerBase
    import inference
    from processing_paligemma import PaliGemmaProcessor
    cfg = MF.write_model_dir(str(tmp_path / "model"))
    img = MF.write_image(str(tmp_path / "pic.png"))
    proc = PaliGemmaProcessor(AutoTokenizer.from_pretrained(MF.TOKENIZER_DIR), 16, 56)
    vocab = cfg["text_config"]["vocab_size"]
    seen = []
    real = PreTrainedTokenizerBase.decode

    def decode(self, token_ids, *a, **k):
        seen.append([int(t) for t in token_ids])
        return real(self, token_ids, *a, **k)
    PreTrainedTokenizerBase.decode = decode
    try:
        inference.main(model_path=str(tmp_path / "model"), image_file_path=img, max_tokens_to_generate=16,
                       detect="cat ; dog")
        out_d = capsys.readouterr().out
        ids_d = seen[0]
        seen.clear()
        inference.main(model_path=str(tmp_path / "model"), prompt="what is this", image_file_path=img,
                       max_tokens_to_generate=16, choices="cat|dog")
        out_c = capsys.readouterr().out
        ids_c = seen[0]
    finally:
        PreTrainedTokenizerBase.decode = real
    dfa = proc.detect_grammar(["cat", "dog"], vocab=vocab)
    assert "detect cat ; dog" in out_d
    assert dfa.accepts(ids_d, prefix=True) and len(ids_d) >= 1, ids_d
    tail = out_d[out_d.index("detect cat ; dog"):].splitlines()[1:]
    if dfa.accepts(ids_d):
        H, W = MF.IMAGE_HW
        boxes = proc.parse_detections(ids_d, H, W, grammar=dfa)
        assert len(tail) == max(1, len(boxes))
        for ln, bx in zip(tail, boxes):
            assert re.fullmatch(r"(cat|dog): y [\d.]+\.\.[\d.]+, x [\d.]+\.\.[\d.]+", ln) and ln.startswith(bx["label"]), ln
        assert boxes or tail == ["no detections"]
    else:
        assert len(ids_d) == 16 and tail[0].startswith("no complete detection answer")
    eos = proc.tokenizer.eos_token_id
    assert ids_c in (proc._ids("cat") + [eos], proc._ids("dog") + [eos]), ids_c
    assert ("what is thiscat" in out_c) or ("what is thisdog" in out_c), out_c[-200:]


def test_model_generate_passes_the_grammar_through(tiny):
    """PaliGemmaForConditionalGeneration.generate(grammar=..., grammar_start=...) is the engine's."""
    from oracle import configs as ocfg, synth
    from modeling_paligemma import PaliGemmaConfig, PaliGemmaForConditionalGeneration
    m = PaliGemmaForConditionalGeneration(PaliGemmaConfig(**ocfg.TINY))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.generate_state_dict(ocfg.TINY).items()}, strict=False)
    m.tie_weights()
    m = m.to("cuda").eval()
    s = shared(tiny, 1)
    got = m.generate(s.inp[0], s.inp[1], s.inp[2], max_new_tokens=NEW, stop_token=None, grammar=s.dfa,
                     grammar_start=s.starts)
    assert got.tolist() == m.engine(s.inp[0].device).generate(*s.inp, NEW, stop_token=None, grammar=s.dfa,
                                                              grammar_start=s.starts).tolist()
    assert all(s.dfa.accepts(r, start=st, prefix=True) for r, st in zip(got.tolist(), s.starts))
