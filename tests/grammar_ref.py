"""Constrained decoding: numpy references for pg_dfa_mask / pg_dfa_advance, and a decode loop that applies a grammar on
the host, without the feature under test.

mask_ref and advance_ref are the definitions of include/pghip.h, one line each.  host_loop runs the engine's own
prefill and *unconstrained* eager decode steps, masks the logits each step returns in torch by mask_ref's rule, picks
with the project's own samplers and steps the DFA in Python: generate(..., grammar=...) must give the same ids, exactly
-- the mask is defined bitwise and the sampler is the same kernel on the same bits."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def mask_ref(logits, cls, trans, state):
    """logits fp32 [B][>= V]: a copy with -inf at [b][t] for every row b whose state s is in [0, S) and every t < V with
    trans[s][cls[t]] < 0; every other word is the input's."""
    out = np.array(logits, dtype=np.float32, copy=True)
    S, V = trans.shape[0], cls.shape[0]
    for b, s in enumerate(np.asarray(state).tolist()):
        if 0 <= s < S:
            out[b, :V][trans[s][cls] < 0] = NEG_INF
    return out


def advance_ref(state, ids, cls, trans):
    """(new states int32 [B], err): a row whose state is in [0, S) moves to trans[s][cls[id]] when that is >= 0; a dead
    token or an id outside [0, V) leaves it and sets err; other rows are free and stay as they are."""
    S, V = trans.shape[0], cls.shape[0]
    out = np.array(state, dtype=np.int32, copy=True)
    err = 0
    for b, (s, t) in enumerate(zip(np.asarray(state).tolist(), np.asarray(ids).tolist())):
        if not 0 <= s < S:
            continue
        n = int(trans[s][cls[t]]) if 0 <= t < V else -1
        if n >= 0:
            out[b] = n
        else:
            err = 1
    return out, err


def host_loop(engine, inputs, dfa, starts, n, sampler=None):
    """n tokens per row of `inputs` = (input_ids, pixel_values, attention_mask) (device tensors) under `dfa` from the
    start states `starts` (-1: a free row), decoded WITHOUT generate's grammar support: prefill_request, a decode state
    without a sampler, eager decode_step(..., sampler=None); each step's logits are masked here, the token is picked
    by ops.argmax (sampler None) or ops.topp_sample (sampler = dict(temperature, top_p, uniforms [n + 1][B])) into
    st["ids"], and the DFA is stepped on the host.  Returns (ids [B][n] as lists, the states before each pick
    [n][B])."""
    import torch
    from pghip import ops
    from pghip.grammar import DEAD
    ids, px, mask = inputs
    B = ids.shape[0]
    V = engine.w.vocab
    cache, feats, logits, nxt = engine.prefill_request(ids, px, mask, n)
    st = engine.decode_state(B, cache, nxt, n, sampler=None)
    assert not st["chain"]
    cls_t = torch.from_numpy(dfa.cls.astype(np.int64)).cuda()
    live = torch.from_numpy(dfa.trans >= 0).cuda()
    state = [int(s) for s in starts]
    seen = []
    if sampler is not None:
        uniforms = sampler["uniforms"].to(device="cuda", dtype=torch.float32).contiguous()

    def pick(lg, advance):
        x = lg[:, :V].clone()
        for b, s in enumerate(state):
            if 0 <= s < dfa.S:
                x[b].masked_fill_(~live[s][cls_t], float("-inf"))          # mask_ref's rule
        kw = dict(hist=st["hist"], step=st["step"])
        if advance:
            kw.update(pos=st["pos"], kv_len=None if st["ragged"] else st["kv_len"])
        if sampler is None:
            ops.argmax(x, st["ids"], st["ws"], **kw)
        else:
            ops.topp_sample(x, st["ids"], uniforms, temperature=sampler["temperature"], top_p=sampler["top_p"], **kw)
        seen.append(list(state))
        for b, t in enumerate(st["ids"].tolist()):
            state[b] = dfa.step(state[b], t)
            assert state[b] != DEAD, (b, t, seen[-1][b])

    pick(logits, False)
    for _ in range(n - 1):
        pick(engine.decode_step(st, cache, feats, None), True)
    return st["hist"][:n].t().cpu().tolist(), seen
