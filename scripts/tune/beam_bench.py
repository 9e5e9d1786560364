"""Beam search: pg_beam_select against torch, and a graph-replayed beam step against a plain greedy step.
    python scripts/tune/beam_bench.py [--out profiles/beam_ab.jsonl]

Each comparison in interleaved pairs (A, B, A, B, ... in one process, so both arms see the same machine state) after a
warm-up of both arms; HIP events over REPS back-to-back calls per round, median and minimum over ROUNDS.

  select   pg_beam_select on [16][257216] (2 prompts x 8 beams) and [4][257216] (1 x 4) fp32 logits against the torch
           composition on the same tensor: log_softmax + add cum + topk over each prompt's W * V candidates.  The
           buffer is re-read call after call, so both arms run cache-warm -- the case of the decode step, where the
           selection follows the lm_head that wrote the logits.  Ids, parents and scores are compared first.
  step     pt-224 synthetic weights, one 8-token prompt after the 256 image tokens.  A: one graph-replayed beam step,
           B = 1, W = 4 (embed, 18 layers, lm_head, pg_beam_select, pg_kv_beam_gather).  B: one graph-replayed greedy
           step of generate on 4 rows of the same prompt (chained argmax + embed): the same layer route.  Every round
           resets both states to START generated tokens and replays REPS steps, so the gather moves START .. START +
           REPS generated keys per row (two to three 32-key blocks).  Also timed alone, back to back on the stream:
           the selection, and the gather with every row taking another row's suffix (a 4-cycle, the most it moves).

One JSON record per comparison, appended to --out."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "paligemma-multimodal-system_amd")]
import torch  # noqa: E402
from pghip import configs, engine, ops, synthetic, weights  # noqa: E402
import bench  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "15"))
REPS = int(os.environ.get("REPS", "24"))
START, NEW = 40, 128
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
assert torch.cuda.is_available(), "beam_bench needs the HIP device"


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


def pairs(arm_a, arm_b, timer):
    for fn in (arm_a, arm_b):
        timer(fn)
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(timer(arm_a))
        tb.append(timer(arm_b))
    return ta, tb


def record(name, unit, ta, tb, **extra):
    rec = dict(bench=name, unit=unit, rounds=ROUNDS, reps=REPS, device=torch.cuda.get_device_name(0),
               new_median=round(statistics.median(ta), 3), new_min=round(min(ta), 3),
               old_median=round(statistics.median(tb), 3), old_min=round(min(tb), 3),
               old_over_new_median=round(statistics.median(tb) / statistics.median(ta), 3), **extra)
    print(json.dumps(rec), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")


# ------------------------------------------------------------------------------------------ (a) pg_beam_select
V = 257216
for B, W in ((2, 8), (1, 4)):
    rows = B * W
    g = torch.Generator().manual_seed(rows)
    logits = (torch.randn(rows, V, generator=g) * 3).cuda()
    cum0 = (-torch.rand(rows, generator=g) * 5).cuda()
    fin0 = torch.zeros(rows, dtype=torch.int32, device="cuda")
    cum, fin = cum0.clone(), fin0.clone()
    ids = torch.empty(rows, dtype=torch.int64, device="cuda")
    par = torch.empty(rows, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.beam_select_workspace(rows, W), dtype=torch.uint8, device="cuda")

    def new_kernel():
        ops.beam_select(logits, cum, fin, ids, par, ws, W=W, stop_token=None)

    def torch_route():
        sc = (torch.log_softmax(logits, -1) + cum0[:, None]).view(B, W * V)
        top, idx = sc.topk(W, dim=-1)
        return top.reshape(-1), (idx % V).reshape(-1), (idx // V + torch.arange(B, device="cuda")[:, None] * W).reshape(-1)

    new_kernel()
    top, tid, tpar = torch_route()
    torch.cuda.synchronize()
    assert torch.equal(ids, tid) and torch.equal(par.long(), tpar) and float((cum - top).abs().max()) < 1e-4
    cum.copy_(cum0)

    def reset():                # (the scores feed back: start every window from the same ones)
        cum.copy_(cum0)

    ta, tb = pairs(new_kernel, torch_route, lambda fn: events_us(fn, before=reset))
    record("beam_select_vs_torch", "us", ta, tb, rows=rows, prompts=B, beams=W, vocab=V,
           cache="warm (same buffer every call)",
           logits_GBps_new=round(rows * V * 4 / (statistics.median(ta) * 1e-6) / 1e9, 1))

# --------------------------------------------------------------------------- (b) a beam step against a greedy step
cfg = configs.CONFIGS["pt-224"]
eng = engine.PaliGemmaEngine(cfg, weights.PackedWeights(cfg, synthetic.SyntheticStateDict(cfg).__getitem__))
prompt = [2, 651, 4906, 603, 476, 2121, 576, 108]
ids1, px1 = bench.synthetic_inputs(cfg, 1, prompt)
ids1, px1 = ids1.cuda(), px1.cuda()
W = 4
L = ids1.shape[1]

# the beam arm
st_b, cache_b, feats_b, samp_b = eng.beam_begin(ids1, px1, torch.ones_like(ids1), NEW, W, stop_token=None)
bm = samp_b["beam"]
beam_step = eng._graph_step(st_b, cache_b, feats_b, samp_b)
graph_b = eng.graphs["decode"]
# the greedy arm: generate's own set-up on 4 rows of the prompt
ids4, px4 = ids1.repeat(W, 1), px1.repeat(W, 1, 1, 1)
cache_g, feats_g, logits_g, nxt_g = eng.prefill_request(ids4, px4, torch.ones_like(ids4), NEW)
samp_g = dict(do_sample=False, temperature=1.0, top_p=1.0)
st_g = eng.decode_state(W, cache_g, nxt_g, NEW, sampler=samp_g)
eng.sample(logits_g, st_g, samp_g, advance=False, feats=feats_g)
greedy_step = eng._graph_step(st_g, cache_g, feats_g, samp_g)
# run both to START generated tokens, then snapshot the states every round starts from (one arm after the other: the
# chained greedy step finds its input rows where its own last step left them, in a buffer the beam step also uses)
for step in (beam_step, greedy_step):
    for _ in range(START - 1):
        step()
torch.cuda.synchronize()
keys = ("ids", "pos", "kv_len", "step")
snap_b = {k: st_b[k].clone() for k in keys}
snap_bm = {k: bm[k].clone() for k in ("cum", "finished", "parent")}
snap_g = {k: st_g[k].clone() for k in keys}
res_g = eng._ws["d_res_a"][: W * eng.w.hidden].clone()      # the chained greedy step's input rows


def reset_b():
    for k, v in snap_b.items():
        st_b[k].copy_(v)
    for k, v in snap_bm.items():
        bm[k].copy_(v)


def reset_g():
    for k, v in snap_g.items():
        st_g[k].copy_(v)
    eng._ws["d_res_a"][: res_g.numel()].copy_(res_g)


def timer(fn):
    return events_us(fn, before=reset_b if fn is beam_step else reset_g)


ta, tb = pairs(beam_step, greedy_step, timer)
moved = float((bm["hist_parent"][START:START + REPS] !=
               torch.arange(W, device="cuda", dtype=torch.int32)[None]).float().mean())

# the two new launches alone, back to back on the stream, at the state after the timed window
reset_b()
for _ in range(REPS // 2):
    beam_step()
torch.cuda.synchronize()
logits_b = bm["logits"]
cycle = torch.tensor([1, 2, 3, 0], dtype=torch.int32, device="cuda")
t_sel, t_gat = [], []
for _ in range(ROUNDS):
    keep = {k: bm[k].clone() for k in ("cum", "finished", "parent")}
    t_sel.append(events_us(lambda: ops.beam_select(logits_b, bm["cum"], bm["finished"], st_b["ids"], bm["parent"],
                                                   bm["ws"], W=W, V=eng.w.vocab, stop_token=None)))
    for k, v in keep.items():
        bm[k].copy_(v)
    t_gat.append(events_us(lambda: ops.kv_beam_gather(cache_b.k, cache_b.vt, cache_b.kd, cache_b.vd, cycle, bm["base"],
                                                      st_b["kv_len"], bm["scratch"], kv_heads=cache_b.kv_heads,
                                                      len_rows=False, len_base=0, S_scr=bm["S_scr"])))
sel, gat = statistics.median(t_sel), statistics.median(t_gat)
step_new, step_old = statistics.median(ta), statistics.median(tb)
record("beam_step_vs_greedy_step", "us", ta, tb, config="pt-224", prompts=1, beams=W, greedy_rows=W, prompt_rows=L,
       generated_keys=[START, START + REPS], rows_reordered_share=round(moved, 3),
       step_overhead_us=round(step_new - step_old, 2),
       select_alone_us=round(sel, 2), gather_4cycle_alone_us=round(gat, 2),
       select_plus_gather_share_of_step=round((sel + gat) / step_new, 4),
       gather_window_keys=int(-(-(L + START + REPS // 2) // 32) * 32 - L // 32 * 32))
