"""Constrained decoding, host side (no GPU): the TokenDFA builders and checks of pghip/grammar.py, the processor's
detect / choices grammars and detection parser on the offline tokenizer (tests/golden/tokenizer), the references of
tests/grammar_ref.py against the DFA's own helpers, generate's argument checks and the CLI's flag conflicts."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grammar_ref as GR
from pghip.grammar import DEAD, FREE, TokenDFA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 1


def _edits(seq, vocab):
    """Every one-token edit of seq: each deletion, each substitution and each insertion (over a few ids that cover the
    grammar's tokens and some it never uses)."""
    pool = sorted(set(seq) | {0, 2, 3, 9, vocab - 1})
    out = set()
    for i in range(len(seq)):
        out.add(tuple(seq[:i] + seq[i + 1:]))
        for t in pool:
            out.add(tuple(seq[:i] + [t] + seq[i + 1:]))
    for i in range(len(seq) + 1):
        for t in pool:
            out.add(tuple(seq[:i] + [t] + seq[i:]))
    return out


# ------------------------------------------------------------------------------------------------ from_choices
def test_from_choices_accepts_exactly_the_choices():
    choices = [[5, 6], [5, 7, 8], [5], [9, 9, 4]]                   # [5] is a prefix of two others
    d = TokenDFA.from_choices(choices, EOS, 40)
    assert d.cls.dtype == np.int16 and d.trans.dtype == np.int16 and d.cls.shape == (40,)
    want = {tuple(c + [EOS]) for c in choices}
    for w in want:
        assert d.accepts(list(w)), w
        assert d.accepts(list(w) + [EOS, EOS]), w                   # the final state's self-loop
        assert not d.accepts(list(w[:-1])) and d.accepts(list(w[:-1]), prefix=True)
    for w in want:
        for e in _edits(list(w), 40):
            if e in want or (e[:-1] in want and e[-1] == EOS):      # (an edit that is another choice, or one more eos)
                continue
            assert not d.accepts(list(e)), (w, e)
    # the node after [5] allows eos and both continuations, nothing else
    s, n = d.walk([5])
    assert n == 1 and sorted(np.nonzero(d.allowed(s))[0].tolist()) == [EOS, 6, 7]
    # the final state allows eos alone
    term, _ = d.walk([5, EOS])
    assert term in d.final and np.nonzero(d.allowed(term))[0].tolist() == [EOS]
    assert d.step(term, EOS) == term and d.step(term, 5) == DEAD
    assert d.step(FREE, 17) == FREE and bool(d.allowed(FREE).all()) and d.accepts([3, 3, 3], start=FREE)


def test_from_choices_rejects_bad_input():
    for bad in ([], [[]], [[5, EOS]], [[5, 40]], [[-1]]):
        with pytest.raises(ValueError):
            TokenDFA.from_choices(bad, EOS, 40)
    with pytest.raises(ValueError):
        TokenDFA.from_choices([[5]], 40, 40)


# ------------------------------------------------------------------------------------------------ detect (tokenizer)
@pytest.fixture(scope="module")
def proc():
    from transformers import AutoTokenizer
    from processing_paligemma import PaliGemmaProcessor
    tok = AutoTokenizer.from_pretrained(os.path.join(ROOT, "tests", "golden", "tokenizer"))
    return PaliGemmaProcessor(tok, num_image_tokens=16, image_size=56)


def _loc(proc, *n):
    return proc.tokenizer.convert_tokens_to_ids([f"<loc{i:04d}>" for i in n])


def test_detect_grammar_on_the_offline_tokenizer(proc):
    tok = proc.tokenizer
    d = proc.detect_grammar(["cat", "dog"])
    eos = tok.eos_token_id
    cat, dog, bird_ok = proc._ids(" cat"), proc._ids(" dog"), proc._ids(" what")
    sep = proc._ids(" ;")
    assert d.cls.shape == (len(tok),) and d.meta["labels"] == ["cat", "dog"]
    l0, l1023 = _loc(proc, 0, 1023)
    assert d.cls[l0] == d.cls[l1023] != 0
    assert len({int(d.cls[i]) for i in _loc(proc, *range(1024))}) == 1
    box = lambda a, b, c, e, lab: _loc(proc, a, b, c, e) + lab  # noqa: E731
    b1, b2, b3 = box(0, 1, 2, 3, cat), box(1023, 0, 512, 7, dog), box(5, 5, 5, 5, cat)
    assert d.accepts([eos])                                                  # no detection
    assert d.accepts(b1 + [eos])
    assert d.accepts(b1 + sep + b2 + [eos])
    assert d.accepts(b1 + sep + b2 + sep + b3 + [eos])
    assert not d.accepts(b1) and d.accepts(b1, prefix=True)                  # cut short: a prefix only
    assert not d.accepts(_loc(proc, 1, 2, 3) + cat + [eos])                  # three <loc> then a label
    assert not d.accepts(_loc(proc, 1, 2, 3, 4, 5) + cat + [eos])            # a fifth <loc>
    assert not d.accepts(_loc(proc, 1, 2, 3, 4) + bird_ok + [eos])           # a label not offered
    assert not d.accepts(_loc(proc, 1, 2, 3) + tok.convert_tokens_to_ids(["<seg005>"]) + cat + [eos])
    assert not d.accepts(tok.convert_tokens_to_ids(["<seg000>"]) + [eos])    # a <seg> token
    assert not d.accepts(b1 + b2 + [eos])                                    # a missing separator
    assert not d.accepts(b1 + sep + [eos])                                   # a separator and no box
    assert not d.accepts(_loc(proc, 1, 2) + [eos])                           # eos inside a box
    assert not d.accepts(_loc(proc, 1, 2, 3, 4) + [eos])                     # ... and before the label
    # the position of the first refused token
    assert d.walk(_loc(proc, 1, 2, 3) + cat + [eos])[1] == 3
    assert d.walk(b1 + b2 + [eos])[1] == len(b1)
    # a model vocabulary larger than the tokenizer: the extra ids are never allowed
    big = proc.detect_grammar(["cat"], vocab=len(tok) + 64)
    assert big.cls.shape == (len(tok) + 64,) and not big.cls[len(tok):].any()
    # ... and one that stops inside the <loc> range (the TINY test model): the <loc> ids below it are the class
    small = proc.detect_grammar(["cat"], vocab=300)
    assert small.cls.shape == (300,) and small.cls[l0] == small.cls[299] != 0 and small.meta["loc_ids"][1023] == l1023
    assert small.accepts(_loc(proc, 0, 149, 7, 7) + cat + [eos]) and not small.accepts(_loc(proc, 0, 150, 7, 7) + cat + [eos])
    assert proc.parse_detections(_loc(proc, 0, 149, 7, 7) + cat + [eos], 1024, 2048)[0]["box"] == (0.0, 298.0, 7.0, 14.0)
    proc.detect_grammar(["cat", "dog"])
    for bad in ([], ["cat", ""], ["zebra"]):                                 # (zebra: <unk> on this tokenizer)
        with pytest.raises(ValueError):
            proc.detect_grammar(bad)


def test_detect_label_that_is_a_prefix_of_another(proc):
    d = proc.detect_grammar(["cat", "cat dog"])
    eos = proc.tokenizer.eos_token_id
    locs = _loc(proc, 1, 2, 3, 4)
    assert d.accepts(locs + proc._ids(" cat") + [eos])
    assert d.accepts(locs + proc._ids(" cat dog") + [eos])
    assert d.accepts(locs + proc._ids(" cat") + proc._ids(" ;") + locs + proc._ids(" cat dog") + [eos])
    assert not d.accepts(locs + proc._ids(" cat cat") + [eos])
    got = proc.parse_detections(locs + proc._ids(" cat") + proc._ids(" ;") + locs + proc._ids(" cat dog") + [eos], 10, 10)
    assert [g["label"] for g in got] == ["cat", "cat dog"]


def test_choices_grammar(proc):
    eos = proc.tokenizer.eos_token_id
    d = proc.choices_grammar(["cat", "dog", "what is this"])
    assert d.cls.shape == (len(proc.tokenizer),)
    for c in ("cat", "dog", "what is this"):
        assert d.accepts(proc._ids(c) + [eos]), c
    assert not d.accepts(proc._ids("what is") + [eos]) and not d.accepts(proc._ids("cat dog") + [eos])
    assert not d.accepts(proc._ids(" cat") + [eos])                          # tokenised as given, no leading space
    with pytest.raises(ValueError):
        proc.choices_grammar(["cat", " "])


# ------------------------------------------------------------------------------------------------ validate
def _small():
    cls = np.array([0, 1, 2, 1], dtype=np.int16)
    trans = np.array([[-1, 1, -1], [-1, -1, 1]], dtype=np.int16)
    return cls, trans


def test_validate():
    cls, trans = _small()
    TokenDFA(cls, trans, final=(1,))                                         # the base table is valid
    t = trans.copy()
    t[1, 2] = -1
    with pytest.raises(ValueError, match="allows no token"):                 # a reachable state with no allowed class
        TokenDFA(cls, t)
    t2 = np.concatenate([trans, np.full((1, 3), -1, np.int16)])              # ... an unreachable one is legal
    TokenDFA(cls, t2)
    t = trans.copy()
    t[0, 0] = 1
    with pytest.raises(ValueError, match="class 0"):                         # class 0 live
        TokenDFA(cls, t)
    with pytest.raises(ValueError, match="4097"):                            # C > 4096
        TokenDFA(np.zeros(8, np.int16), np.full((1, 4097), -1, np.int16))
    with pytest.raises(ValueError, match="32768"):                           # S > 32767
        TokenDFA(cls, np.full((32768, 3), -1, np.int16))
    with pytest.raises(ValueError, match="int16"):                           # wrong dtypes
        TokenDFA(cls.astype(np.int32), trans)
    with pytest.raises(ValueError, match="int16"):
        TokenDFA(cls, trans.astype(np.int64))
    with pytest.raises(ValueError):                                          # C < 2
        TokenDFA(np.zeros(4, np.int16), np.full((1, 1), -1, np.int16))
    with pytest.raises(ValueError, match="used by no token"):                # a class no token has
        TokenDFA(np.array([0, 1, 1, 1], np.int16), trans)
    with pytest.raises(ValueError):                                          # a class outside [0, C)
        TokenDFA(np.array([0, 1, 3, 1], np.int16), trans)
    t = trans.copy()
    t[0, 1] = 2
    with pytest.raises(ValueError):                                          # a next state outside [-1, S)
        TokenDFA(cls, t)
    with pytest.raises(ValueError):                                          # a start state outside [0, S)
        TokenDFA(cls, trans, starts=(2,))
    with pytest.raises(ValueError):
        TokenDFA(cls[:, None], trans)
    d = TokenDFA(cls.astype(np.int32), trans, validate=False)                # the builders call validate(); so can a user
    with pytest.raises(ValueError):
        d.validate()


# ------------------------------------------------------------------------------------------------ union
def test_union_members_accept_what_they_accepted_alone(proc):
    a = TokenDFA.from_choices([[5, 6], [5, 7, 8]], EOS, len(proc.tokenizer))
    b = proc.detect_grammar(["cat", "dog"])
    c = TokenDFA.from_choices([[14], [6, 5]], EOS, len(proc.tokenizer))
    u = TokenDFA.union([a, b, c])
    assert u.starts == (0, a.S + b.start, a.S + b.S) and u.S == a.S + b.S + c.S
    with pytest.raises(ValueError):
        u.start                                                              # a union has no single start state
    eos = EOS
    probes = [[5, 6, eos], [5, 7, 8, eos], [5, 7, eos], [6, 5, eos], [14, eos], [eos], [5], [6], [14, 14, eos],
              _loc(proc, 1, 2, 3, 4) + proc._ids(" cat") + [eos], _loc(proc, 1, 2, 3) + proc._ids(" cat") + [eos],
              _loc(proc, 1, 2, 3, 4) + proc._ids(" dog ;") + _loc(proc, 9, 9, 9, 9) + proc._ids(" cat") + [eos]]
    rng = np.random.default_rng(0)
    probes += [rng.choice([1, 5, 6, 7, 8, 14, 15, 9, 150], size=rng.integers(1, 6)).tolist() for _ in range(300)]
    hits = [0, 0, 0]
    for p in probes:
        for i, (m, s) in enumerate(zip((a, b, c), u.starts)):
            assert u.accepts(p, start=s) == m.accepts(p), (p, i)
            assert u.walk(p, start=s)[1] == m.walk(p)[1], (p, i)
            hits[i] += m.accepts(p)
    assert min(hits) >= 2
    with pytest.raises(ValueError):
        TokenDFA.union([a, TokenDFA.from_choices([[5]], EOS, 40)])           # different vocabularies
    with pytest.raises(ValueError):
        TokenDFA.union([])


# ------------------------------------------------------------------------------------------------ parse_detections
def test_parse_detections_round_trip(proc):
    d = proc.detect_grammar(["cat", "dog"])
    eos = proc.tokenizer.eos_token_id
    H, W = 480, 640
    boxes = [("cat", (0, 256, 512, 1023)), ("dog", (100, 1, 101, 2)), ("cat", (1023, 1023, 0, 0))]
    ids = []
    for i, (lab, q) in enumerate(boxes):
        ids += (proc._ids(" ;") if i else []) + _loc(proc, *q) + proc._ids(" " + lab)
    ids.append(eos)
    want = [{"label": lab, "box": (q[0] / 1024 * H, q[1] / 1024 * W, q[2] / 1024 * H, q[3] / 1024 * W)}
            for lab, q in boxes]
    assert want[0]["box"] == (0.0, 160.0, 240.0, 1023 / 1024 * 640)
    for form in (ids, torch.tensor([ids]), np.array(ids)):
        assert proc.parse_detections(form, H, W) == want
    assert proc.parse_detections(ids, H, W, grammar=d) == want
    text = "<loc0000><loc0256><loc0512><loc1023> cat ;<loc0100><loc0001><loc0101><loc0002> dog"
    assert proc.parse_detections(text, H, W) == want[:2]                     # text: tokenised again, <eos> supplied
    assert proc.parse_detections([eos], H, W) == []
    # malformed: the error names the position of the first token the grammar refuses
    bad = _loc(proc, 1, 2, 3) + proc._ids(" cat") + [eos]
    with pytest.raises(ValueError, match="position 3"):
        proc.parse_detections(bad, H, W)
    with pytest.raises(ValueError, match=f"position {len(ids) - 1}"):        # cut before its <eos>
        proc.parse_detections(ids[:-1], H, W)
    with pytest.raises(ValueError, match="position 0"):
        proc.parse_detections(proc._ids("cat"), H, W)
    with pytest.raises(ValueError):                                          # not a detect grammar
        proc.parse_detections(ids, H, W, grammar=proc.choices_grammar(["cat"]))


# ------------------------------------------------------------------------------------------------ references
def test_references_agree_with_the_dfa_helpers(proc):
    d = proc.detect_grammar(["cat", "dog"])
    rng = np.random.default_rng(1)
    V = d.vocab
    states = np.array([-1, d.S, d.start, d.meta["label_state"], d.meta["box_state"], 1, d.S + 9], dtype=np.int32)
    x = rng.standard_normal((len(states), V + 3)).astype(np.float32)
    x[2, 5] = np.nan
    got = GR.mask_ref(x, d.cls, d.trans, states)
    for b, s in enumerate(states.tolist()):
        ok = d.allowed(s) if 0 <= s < d.S else np.ones(V, bool)
        assert np.array_equal(got[b, :V][ok].view(np.int32), x[b, :V][ok].view(np.int32))
        assert bool(np.isneginf(got[b, :V][~ok]).all())
        assert np.array_equal(got[b, V:], x[b, V:])
    ids = np.array([7, 7, _loc(proc, 3)[0], proc._ids(" cat")[0], 7, EOS, 7], dtype=np.int64)
    new, err = GR.advance_ref(states, ids, d.cls, d.trans)
    for b, (s, t) in enumerate(zip(states.tolist(), ids.tolist())):
        n = d.step(s, t) if 0 <= s < d.S else s
        assert new[b] == (s if n == DEAD else n)
    assert err == 1                                                          # row 4: token 7 in the box state
    assert GR.advance_ref(states[:4], ids[:4], d.cls, d.trans)[1] == 0
    new, err = GR.advance_ref(np.array([0], np.int32), np.array([V]), d.cls, d.trans)   # an id outside [0, V)
    assert new.tolist() == [0] and err == 1


# ------------------------------------------------------------------------------------------------ generate's checks
def _cpu_engine():
    from pghip import engine
    eng = object.__new__(engine.PaliGemmaEngine)
    eng.w = SimpleNamespace(vocab=300)
    eng.tp = 1

    def never(*a, **k):
        raise AssertionError("a launch was reached")
    eng.prefill_request = never
    eng.decode_state = never
    return eng


def test_generate_rejects_bad_grammar_arguments_before_any_launch():
    eng = _cpu_engine()
    ids = torch.zeros(2, 5, dtype=torch.int64)
    ok = TokenDFA.from_choices([[5, 6]], EOS, 300)
    for kw in (dict(grammar=TokenDFA.from_choices([[5, 6]], EOS, 299)),      # cls of the wrong length
               dict(grammar=ok, grammar_start=ok.S), dict(grammar=ok, grammar_start=-2),
               dict(grammar=ok, grammar_start=[0, ok.S]), dict(grammar=ok, grammar_start=[0]),
               dict(grammar=ok, grammar_start=[0, 0, 0]), dict(grammar=ok, grammar_start=0.0),
               dict(grammar=TokenDFA.union([ok, ok])),                       # two start states and none named
               dict(grammar_start=0)):
        with pytest.raises(ValueError):
            eng.generate(ids, None, torch.ones_like(ids), 4, **kw)
    eng.tp = 2
    with pytest.raises(NotImplementedError):
        eng.generate(ids, None, torch.ones_like(ids), 4, grammar=ok)
    eng.tp = 1
    with pytest.raises(AssertionError, match="a launch was reached"):        # valid arguments do go on
        eng.generate(ids, None, torch.ones_like(ids), 4, grammar=ok, grammar_start=[-1, 0])
    assert eng.grammar_args(ok, None, 3, 300) == [0, 0, 0] and eng.grammar_args(None, None, 3, 300) is None
    u = TokenDFA.union([ok, ok])
    assert eng.grammar_args(u, [u.starts[1], -1], 2, 300) == [u.starts[1], -1]


def test_public_signatures_and_bindings():
    from modeling_paligemma import PaliGemmaForConditionalGeneration as M
    from pghip import _lib, engine, ops
    for fn in (M.generate, engine.PaliGemmaEngine.generate):
        p = inspect.signature(fn).parameters
        assert p["grammar"].default is None and p["grammar_start"].default is None
    assert "grammar" not in inspect.signature(engine.PaliGemmaEngine.generate_beam).parameters
    assert _lib.ABI_VERSION == 13
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pghip.h")).read(), flags=re.S)
    for name in ("pg_dfa_mask", "pg_dfa_advance"):
        m = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert callable(ops.dfa_mask) and callable(ops.dfa_advance)
    assert ops.DFA_MAX_STATES == 32767 and ops.DFA_MAX_CLASSES == 4096 and ops.DFA_MAX_ROWS == 1024


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_flag_conflicts_raise_before_any_model_is_loaded(monkeypatch):
    import inference

    def never(*a, **k):
        raise AssertionError("the model was loaded")
    monkeypatch.setattr(inference, "load_hf_model", never)
    base = ["--model_path", "nowhere", "--image_file_path", "none.png"]
    for extra in (["--detect", "cat ; dog", "--num_beams", "2"],
                  ["--prompt", "what is this", "--choices", "yes|no", "--num_beams", "2"],
                  ["--detect", "cat", "--choices", "yes|no"],
                  ["--detect", "cat ; ; dog"], ["--prompt", "q", "--choices", "yes||no"],
                  ["--detect", "cat", "--prompt", "detect cat"]):
        with pytest.raises(ValueError):
            inference._cli(base + extra)
    assert inference.detect_prompt("cat ; dog") == "detect cat ; dog"
    assert inference.detect_prompt(" cat;dog ;  what is this ") == "detect cat ; dog ; what is this"
    assert inference.detect_labels("cat ; dog") == ["cat", "dog"]
    assert inference.choice_list("yes|no| unsure") == ["yes", "no", "unsure"]
    p = inspect.signature(inference.main).parameters
    assert p["detect"].default is None and p["choices"].default is None
