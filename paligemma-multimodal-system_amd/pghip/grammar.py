"""Grammars for constrained decoding, as data: a DFA over token classes (host side, pure Python / numpy).

A TokenDFA is two int16 tables:

    cls   [V]      the class of every token id; class 0 is "never allowed"
    trans [S][C]   the next state, or -1 for "not allowed here"; trans[s][0] == -1 for every s

so token t is allowed in state s iff trans[s][cls[t]] >= 0 -- no per-state bitmask over the vocabulary exists.  Tokens
the grammar treats alike (all 1024 <loc> tokens, say) share a class, which keeps C small: the device turns one row of
trans into a C-bit bitmap (csrc/grammar.hip).  S <= 32767 and 2 <= C <= 4096.

A decoding row's state is one int32.  State -1 (FREE) means the row is unconstrained and stays so, which lets
constrained and unconstrained rows share a batch.  `final` marks the states reached by the end token: accepts() asks
for one of them, the device never reads it.

Limitation (detect_grammar / choices_grammar of PaliGemmaProcessor): a label or choice is accepted only in the
tokenisation the tokenizer gives for it, not in every token sequence that decodes to the same text.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence

import numpy as np

FREE = -1          # a row's state: unconstrained, and stays so
DEAD = -2          # step()'s answer for a token the state does not allow
MAX_STATES = 32767
MAX_CLASSES = 4096


class _Tables:
    """What the builders share: token -> class, and states as {class: next state}."""

    def __init__(self, vocab: int):
        if not isinstance(vocab, (int, np.integer)) or vocab < 1:
            raise ValueError(f"vocab must be a positive integer, got {vocab!r}")
        self.vocab = int(vocab)
        self.cls_of = {}
        self.n_cls = 1                  # class 0: never allowed
        self.rows: List[dict] = []

    def _tok(self, t) -> int:
        if not isinstance(t, (int, np.integer)) or not 0 <= int(t) < self.vocab:
            raise ValueError(f"token id {t!r} outside the vocabulary [0, {self.vocab})")
        return int(t)

    def klass(self, tok) -> int:
        """The class of one token: its own, made on first use."""
        tok = self._tok(tok)
        if tok not in self.cls_of:
            self.cls_of[tok] = self.n_cls
            self.n_cls += 1
        return self.cls_of[tok]

    def klass_set(self, toks: Iterable) -> int:
        """One new class for a set of tokens, none of which may have a class yet."""
        toks = [self._tok(t) for t in toks]
        if not toks:
            raise ValueError("a token class needs at least one token")
        for t in toks:
            if t in self.cls_of:
                raise ValueError(f"token id {t} would belong to two classes")
        for t in toks:
            self.cls_of[t] = self.n_cls
        self.n_cls += 1
        return self.n_cls - 1

    def state(self) -> int:
        self.rows.append({})
        return len(self.rows) - 1

    def edge(self, s: int, c: int, to: Optional[int] = None) -> int:
        """The state class c leads to from s: the existing one, else `to`, else a new state.  An existing edge to
        another state than `to` makes the grammar ambiguous for a deterministic automaton: ValueError."""
        have = self.rows[s].get(c)
        if have is not None:
            if to is not None and have != to:
                raise ValueError("ambiguous grammar: one token sequence would have to continue in two ways")
            return have
        if to is None:
            to = self.state()
        self.rows[s][c] = to
        return to

    def walk(self, s: int, seq: Sequence, last_to: Optional[int] = None) -> int:
        """Follow / create the trie path of seq from s; the last edge goes to last_to when given."""
        seq = list(seq)
        for i, t in enumerate(seq):
            s = self.edge(s, self.klass(t), last_to if i + 1 == len(seq) else None)
        return s

    def finish(self, starts, final, meta=None) -> "TokenDFA":
        if len(self.rows) > MAX_STATES or self.n_cls > MAX_CLASSES:
            raise ValueError(f"the grammar needs {len(self.rows)} states and {self.n_cls} token classes; a TokenDFA "
                             f"holds at most {MAX_STATES} and {MAX_CLASSES}")
        cls = np.zeros(self.vocab, dtype=np.int16)
        for t, c in self.cls_of.items():
            cls[t] = c
        trans = np.full((len(self.rows), max(2, self.n_cls)), -1, dtype=np.int16)
        for s, row in enumerate(self.rows):
            for c, to in row.items():
                trans[s, c] = to
        return TokenDFA(cls, trans, starts=starts, final=final, meta=meta)


def _seq(seq, what: str) -> list:
    seq = [int(t) for t in (seq.tolist() if hasattr(seq, "tolist") else seq)]
    if not seq:
        raise ValueError(f"{what}: an empty token sequence")
    return seq


class TokenDFA:
    """cls int16 [V], trans int16 [S][C] (module docstring); `starts`: the start states (one per member of a union);
    `final`: the states in which a sequence may end.  The constructor validates unless told otherwise."""

    def __init__(self, cls, trans, starts=(0,), final=(), meta: Optional[dict] = None, validate: bool = True):
        self.cls = cls
        self.trans = trans
        self.starts = tuple(int(s) for s in starts)
        self.final = frozenset(int(s) for s in final)
        self.meta = dict(meta or {})
        if validate:
            self.validate()

    # ---------------------------------------------------------------- shape
    @property
    def vocab(self) -> int:
        return int(self.cls.shape[0])

    @property
    def S(self) -> int:
        return int(self.trans.shape[0])

    @property
    def C(self) -> int:
        return int(self.trans.shape[1])

    @property
    def start(self) -> int:
        """The start state of a grammar that has exactly one."""
        if len(self.starts) != 1:
            raise ValueError(f"this TokenDFA has {len(self.starts)} start states (a union): name one")
        return self.starts[0]

    def live(self) -> np.ndarray:
        """bool [S][C]: class c is allowed in state s."""
        return self.trans >= 0

    # ---------------------------------------------------------------- checks
    def validate(self) -> "TokenDFA":
        """ValueError unless the tables are what the device kernels take: int16 arrays of the right rank, 1 <= S <=
        32767, 2 <= C <= 4096, classes in [0, C), next states in [-1, S), class 0 dead in every state, every other
        class used by some token, start and final states in range, and every state reachable from a start state with
        at least one allowed class (the sampler would be handed a row of nothing but -inf)."""
        cls, trans = self.cls, self.trans
        if not isinstance(cls, np.ndarray) or not isinstance(trans, np.ndarray):
            raise ValueError("cls and trans must be numpy arrays")
        if cls.dtype != np.int16 or trans.dtype != np.int16:
            raise ValueError(f"cls and trans must be int16, got {cls.dtype} and {trans.dtype}")
        if cls.ndim != 1 or trans.ndim != 2 or cls.shape[0] < 1:
            raise ValueError(f"cls must be [V] and trans [S][C], got {cls.shape} and {trans.shape}")
        S, C = trans.shape
        if not 1 <= S <= MAX_STATES:
            raise ValueError(f"S = {S} states, outside [1, {MAX_STATES}]")
        if not 2 <= C <= MAX_CLASSES:
            raise ValueError(f"C = {C} token classes, outside [2, {MAX_CLASSES}]")
        if int(cls.min()) < 0 or int(cls.max()) >= C:
            raise ValueError(f"a token class outside [0, {C})")
        if int(trans.min()) < -1 or int(trans.max()) >= S:
            raise ValueError(f"a next state outside [-1, {S})")
        if bool((trans[:, 0] != -1).any()):
            raise ValueError(f"class 0 (never allowed) is allowed in state {int(np.nonzero(trans[:, 0] != -1)[0][0])}")
        used = np.zeros(C, dtype=bool)
        used[cls] = True
        used[0] = True
        if not bool(used.all()):
            raise ValueError(f"class {int(np.nonzero(~used)[0][0])} is used by no token")
        if not self.starts:
            raise ValueError("a TokenDFA needs a start state")
        for s in (*self.starts, *self.final):
            if not 0 <= s < S:
                raise ValueError(f"start / final state {s} outside [0, {S})")
        seen = np.zeros(S, dtype=bool)
        todo = list(self.starts)
        seen[todo] = True
        while todo:
            s = todo.pop()
            nxt = trans[s][trans[s] >= 0]
            if nxt.size == 0:
                raise ValueError(f"state {s} is reachable and allows no token")
            for n in np.unique(nxt).tolist():
                if not seen[n]:
                    seen[n] = True
                    todo.append(n)
        return self

    # ---------------------------------------------------------------- host helpers (tests, the detection parser)
    def step(self, state: int, token: int) -> int:
        """The state after `token`: FREE stays FREE; DEAD when the state does not allow the token (or DEAD came in)."""
        state, token = int(state), int(token)
        if state == FREE:
            return FREE
        if not 0 <= state < self.S or not 0 <= token < self.vocab:
            return DEAD
        n = int(self.trans[state, int(self.cls[token])])
        return n if n >= 0 else DEAD

    def allowed(self, state: int) -> np.ndarray:
        """bool [V]: the tokens `state` allows (all of them for FREE)."""
        if int(state) == FREE:
            return np.ones(self.vocab, dtype=bool)
        return self.trans[int(state)][self.cls] >= 0

    def walk(self, ids, start: Optional[int] = None):
        """(state, n): the state after the longest prefix of ids the grammar allows from `start`, and its length."""
        s = self.start if start is None else int(start)
        ids = [int(t) for t in (ids.tolist() if hasattr(ids, "tolist") else ids)]
        for i, t in enumerate(ids):
            n = self.step(s, t)
            if n == DEAD:
                return s, i
            s = n
        return s, len(ids)

    def accepts(self, ids, start: Optional[int] = None, prefix: bool = False) -> bool:
        """Whether the grammar allows every token of ids from `start` and ends in a final state; prefix=True asks only
        for the former (a sequence cut short by max_new_tokens).  From FREE everything is accepted."""
        s, n = self.walk(ids, start)
        if n != len(ids):
            return False
        return prefix or s == FREE or s in self.final

    # ---------------------------------------------------------------- builders
    @classmethod
    def from_choices(cls, seqs, eos: int, vocab: int) -> "TokenDFA":
        """One of the token sequences `seqs`, then `eos`.  After `eos` a final state allows only `eos` again (a batch
        keeps stepping until every row has stopped; those tokens are cut on the host).  A choice that is a prefix of
        another is legal: its node allows `eos` and the continuation."""
        t = _Tables(vocab)
        seqs = [_seq(s, "from_choices") for s in seqs]
        if not seqs:
            raise ValueError("from_choices: no choice given")
        eos = t._tok(eos)
        if any(eos in s for s in seqs):
            raise ValueError("from_choices: a choice contains the end token")
        root, term = t.state(), t.state()
        ce = t.klass(eos)
        t.edge(term, ce, term)
        for s in seqs:
            t.edge(t.walk(root, s), ce, term)
        return t.finish((root,), (term,), meta={"kind": "choices", "eos": eos})

    @classmethod
    def detect(cls, loc_ids, label_seqs, sep_seq, eos: int, vocab: int) -> "TokenDFA":
        """OUT := eos | BOX (sep BOX)* eos ; BOX := loc loc loc loc LABEL, LABEL one of label_seqs (a trie).  Cyclic:
        no box count is unrolled, max_new_tokens bounds the length.  All loc_ids share one class."""
        t = _Tables(vocab)
        labels = [_seq(s, "detect: label") for s in label_seqs]
        sep = _seq(sep_seq, "detect: separator")
        if not labels:
            raise ValueError("detect: no label given")
        eos = t._tok(eos)
        loc_ids = [int(i) for i in loc_ids]
        cl = t.klass_set(loc_ids)
        if eos in loc_ids or eos in sep or any(eos in s for s in labels):
            raise ValueError("detect: the end token appears in a label, the separator or the <loc> ids")
        if any(i in sep or any(i in s for s in labels) for i in set(loc_ids)):
            raise ValueError("detect: a <loc> id appears in a label or the separator")
        ce = t.klass(eos)
        start, term, box = t.state(), t.state(), t.state()
        t.edge(term, ce, term)
        t.edge(start, ce, term)
        l1 = t.edge(box, cl)
        t.edge(start, cl, l1)
        lab = t.edge(t.edge(t.edge(l1, cl), cl), cl)
        ends = [t.walk(lab, s) for s in labels]
        for e in ends:                      # after a label: the end, or the separator and the next box
            t.edge(e, ce, term)
            t.walk(e, sep, last_to=box)
        return t.finish((start,), (term,), meta={"kind": "detect", "eos": eos, "loc_ids": loc_ids, "label_seqs": labels,
                                                 "label_state": lab,
                                                 "box_state": box, "sep_len": len(sep)})

    @classmethod
    def union(cls, dfas: Sequence["TokenDFA"]) -> "TokenDFA":
        """One table for a batch whose rows follow different grammars: the members' states side by side, member i's
        start states after member i - 1's in `starts`.  Tokens share a joint class iff every member gives them the same
        class."""
        dfas = list(dfas)
        if not dfas:
            raise ValueError("union: no grammar given")
        V = dfas[0].vocab
        if any(d.vocab != V for d in dfas):
            raise ValueError("union: the grammars have different vocabularies")
        keys = np.stack([d.cls for d in dfas], axis=1)                      # [V][k]
        uniq, joint = np.unique(keys, axis=0, return_inverse=True)
        joint = joint.reshape(-1)
        zero = np.nonzero((uniq == 0).all(axis=1))[0]
        if zero.size:                       # np.unique sorts rows: the all-zero tuple, if any token has it, comes first
            assert int(zero[0]) == 0
        else:                               # no token is dead in every member: class 0 stays reserved, and empty
            uniq = np.concatenate([np.zeros((1, len(dfas)), dtype=uniq.dtype), uniq])
            joint = joint + 1
        C = uniq.shape[0]
        S = sum(d.S for d in dfas)
        if S > MAX_STATES or C > MAX_CLASSES:
            raise ValueError(f"union: {S} states and {C} joint token classes; a TokenDFA holds at most {MAX_STATES} "
                             f"and {MAX_CLASSES}")
        trans = np.full((S, C), -1, dtype=np.int16)
        starts, final, off = [], [], 0
        for i, d in enumerate(dfas):
            sub = d.trans[:, uniq[:, i]].astype(np.int32)                   # [S_i][C]: member i's class of each joint class
            trans[off:off + d.S] = np.where(sub >= 0, sub + off, -1).astype(np.int16)
            starts += [s + off for s in d.starts]
            final += [s + off for s in d.final]
            off += d.S
        trans[:, 0] = -1
        return TokenDFA(joint.astype(np.int16), trans, starts=starts, final=final,
                        meta={"kind": "union", "members": [dict(d.meta) for d in dfas]})
