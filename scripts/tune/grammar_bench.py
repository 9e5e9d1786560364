"""Constrained decoding: what pg_dfa_mask + pg_dfa_advance cost, alone, in a decode step, and in the headline.
    python scripts/tune/grammar_bench.py [--out profiles/grammar_ab.jsonl] [--parent DIR] [--only kernels,step,headline]

Each comparison in interleaved pairs (A, B, A, B, ... so both arms see the same machine state) after a warm-up of both
arms; HIP events over REPS back-to-back calls per round, median and minimum over ROUNDS.

  kernels   pg_dfa_mask + pg_dfa_advance on [1][257216] and [16][257216] fp32 logits with the detect grammar's tables
            (built by TokenDFA.detect over a 257216-id vocabulary: 1024 <loc> ids, two labels), every row in the state
            after the fourth <loc> (one label token allowed: nearly the whole row is written).  Against the torch
            expression that does the same in place: logits.masked_fill_(~live[state][:, cls], -inf) plus the state
            gather trans[state, cls[ids]].  The buffer is rewritten call after call, so both arms run cache-warm -- the
            case of the decode step, where the mask follows the lm_head that wrote the logits.  The masked bits are
            compared first.
  step      pt-224 synthetic weights, one 8-token prompt after the 256 image tokens, B = 1: one graph-replayed greedy
            decode step with the detect grammar in the sampler (A) against the same step without (B).  Every round
            resets both states to START generated tokens; the grammar arm also resets its DFA state.
  headline  (--parent DIR: a built checkout of the parent commit)  bench.py --gpus 1 --steps 5 --warmup 2 of this tree
            against DIR's, four interleaved runs each, every run a fresh process; tokens/s, higher is better.

One JSON record per comparison, appended to --out."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "paligemma-multimodal-system_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from pghip import configs, engine, ops, synthetic, weights  # noqa: E402
from pghip.grammar import TokenDFA  # noqa: E402
import bench  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "15"))
REPS = int(os.environ.get("REPS", "24"))
START, NEW = 40, 128
V = 257216


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


out_path = _arg("--out")
parent = _arg("--parent")
only = set(_arg("--only", "kernels,step,headline").split(","))
assert torch.cuda.is_available(), "grammar_bench needs the HIP device"


def events_us(run, reps=REPS, before=None):
    if before is not None:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def pairs(arm_a, arm_b, timer, rounds=ROUNDS):
    for fn in (arm_a, arm_b):
        timer(fn)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timer(arm_a))
        tb.append(timer(arm_b))
    return ta, tb


def record(name, unit, ta, tb, reps=REPS, **extra):
    rec = dict(bench=name, unit=unit, rounds=len(ta), reps=reps, device=torch.cuda.get_device_name(0),
               new_median=round(statistics.median(ta), 3), new_min=round(min(ta), 3),
               old_median=round(statistics.median(tb), 3), old_min=round(min(tb), 3),
               old_over_new_median=round(statistics.median(tb) / statistics.median(ta), 3), **extra)
    print(json.dumps(rec), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def detect_dfa():
    """The detect grammar over a PaliGemma-sized vocabulary: the 1024 <loc> ids where the real tokenizer has them
    (256000 ..), two two-token labels, a one-token separator."""
    return TokenDFA.detect(list(range(256000, 257024)), [[5, 2460], [5, 5929]], [2161], 1, V)


dfa = detect_dfa()
cls_d = torch.from_numpy(dfa.cls).cuda()
trans_d = torch.from_numpy(dfa.trans).cuda()

# ------------------------------------------------------------------------------------------ (1) the two kernels alone
if "kernels" in only:
    live_d = trans_d >= 0
    cls_l = cls_d.long()
    label_state = dfa.meta["label_state"]
    for B in (1, 16):
        g = torch.Generator().manual_seed(B)
        logits0 = (torch.randn(B, V, generator=g) * 3).cuda()
        logits = logits0.clone()
        state0 = torch.full((B,), label_state, dtype=torch.int32, device="cuda")
        state = state0.clone()
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        ids = torch.full((B,), 5, dtype=torch.int64, device="cuda")          # the labels' first token

        def new_kernels():
            ops.dfa_mask(logits, cls_d, trans_d, state0)
            ops.dfa_advance(state, ids, cls_d, trans_d, err)

        tstate = state0.long()

        def torch_route():
            logits.masked_fill_(~live_d[tstate][:, cls_l], float("-inf"))
            return trans_d[tstate, cls_l[ids]]

        new_kernels()
        a = logits.clone()
        s_new = state.clone()
        logits.copy_(logits0)
        s_ref = torch_route()
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), logits.view(torch.int32)) and torch.equal(s_new.long(), s_ref.long())
        assert int(err) == 0

        def reset():                # (the state feeds back: start every window from the same one)
            state.copy_(state0)

        ta, tb = pairs(new_kernels, torch_route, lambda fn: events_us(fn, before=reset))
        dead = int(torch.isneginf(a).sum())
        record("dfa_mask_advance_vs_torch", "us", ta, tb, rows=B, vocab=V, states=dfa.S, classes=dfa.C,
               dead_tokens_per_row=dead // B, cache="warm (same buffer every call)",
               store_GBps_new=round(dead * 4 / (statistics.median(ta) * 1e-6) / 1e9, 1))

# ------------------------------------------------------------------------ (2) a decode step with and without a grammar
if "step" in only:
    cfg = configs.CONFIGS["pt-224"]
    eng = engine.PaliGemmaEngine(cfg, weights.PackedWeights(cfg, synthetic.SyntheticStateDict(cfg).__getitem__))
    prompt = [2, 651, 4906, 603, 476, 2121, 576, 108]
    ids1, px1 = bench.synthetic_inputs(cfg, 1, prompt)
    ids1, px1 = ids1.cuda(), px1.cuda()
    # a grammar every state of which allows every <loc> id (a ring of four states), so that REPS steps from any start
    # stay inside it whatever the synthetic weights prefer
    ring_cls = np.zeros(V, dtype=np.int16)
    ring_cls[256000:257024] = 1
    ring = TokenDFA(ring_cls, np.array([[-1, 1], [-1, 2], [-1, 3], [-1, 0]], dtype=np.int16))
    arms = {}
    for name, gram in (("grammar", ring), ("plain", None)):
        cache, feats, logits_p, nxt = eng.prefill_request(ids1, px1, torch.ones_like(ids1), NEW)
        samp = dict(do_sample=False, temperature=1.0, top_p=1.0)
        st = eng.decode_state(1, cache, nxt, NEW, sampler=samp)
        if gram is not None:
            samp["grammar"] = eng.grammar_state(gram, [0])
        eng.sample(logits_p, st, samp, advance=False, feats=feats)
        step = eng._graph_step(st, cache, feats, samp)
        for _ in range(START - 1):
            step()
        torch.cuda.synchronize()
        snap = {k: st[k].clone() for k in ("ids", "pos", "kv_len", "step")}
        res = eng._ws["d_res_a"][: eng.w.hidden].clone()            # the chained step's input row
        gsnap = samp["grammar"]["state"].clone() if gram is not None else None
        arms[name] = (step, st, samp, snap, res, gsnap)

    def make_reset(name):
        step, st, samp, snap, res, gsnap = arms[name]

        def reset():
            for k, v in snap.items():
                st[k].copy_(v)
            eng._ws["d_res_a"][: res.numel()].copy_(res)
            if gsnap is not None:
                samp["grammar"]["state"].copy_(gsnap)
        return reset

    resets = {arms[n][0]: make_reset(n) for n in arms}
    ta, tb = pairs(arms["grammar"][0], arms["plain"][0], lambda fn: events_us(fn, before=resets[fn]))
    assert int(arms["grammar"][2]["grammar"]["err"]) == 0
    record("decode_step_grammar_vs_plain", "us", ta, tb, config="pt-224", rows=1, generated_keys=[START, START + REPS],
           step_overhead_us=round(statistics.median(ta) - statistics.median(tb), 2))

# ---------------------------------------------------------------------------- (3) the headline against the parent tree
if "headline" in only and parent:
    def headline(tree):
        r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup",
                            "2"], cwd=tree, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"bench.py failed in {tree}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln][-1]
        return float(json.loads(line)["value"])

    ta, tb = [], []
    for _ in range(4):
        ta.append(headline(ROOT))
        tb.append(headline(os.path.abspath(parent)))
        print(f"headline: this tree {ta[-1]:.2f}, parent {tb[-1]:.2f} tokens/s", flush=True)
    record("bench_headline_vs_parent", "tokens/s (higher is better)", ta, tb, reps=1, runs_new=ta, runs_old=tb)
