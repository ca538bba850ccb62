"""What the gradients of K candidate-order scores cost: mmseq_order_score_bwd
(berson.score_orders_grad) against the torch-only route (berson.score_orders_autograd), beside
the encode they hang off and the K full passes the package needed before.

    python tools/order_grad_bench.py [--stories 32] [--rounds 5] [--log profiles/order_grad_bench.log]

Part 1, the config-3 preset (N = 5, H = 768), bf16, train mode, --stories seeded synthetic stories,
K in {8, 32, 120} seeded candidate orders per story (120 = every order). In one process, windows
of one forward + backward each alternate between
  (a) encode alone (backward of a sum over the encoder outputs the decoder reads),
  (b) score_orders_grad on that encoder output, detached (backward of the summed scores),
  (c) score_orders_autograd, likewise,
  (d) one model(inputs) forward / backward; x K is what K labelled passes cost: an EXTRAPOLATION,
every window between two device events; one warm-up round, then the median of --rounds. Peak
allocated memory above the resting level is reported for (b) and (c).

Part 2, the head alone at config 5's N = 9, H = 1024 with B = 8, K = 64 (decoder inputs from
beam_batch_ref.random_case, fp32): the same two routes, time and peak memory.

Nothing is gated on these numbers. Prints one JSON line and writes it to --log.
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import beam_batch_ref as R  # noqa: E402
import bench  # noqa: E402
from multimodal_sequencing_amd import berson, model_zoo  # noqa: E402


def orders_for(B, N, K, seed):
    rng = random.Random(seed)
    return torch.tensor([[rng.sample(range(N), N) for _ in range(K)] for _ in range(B)],
                        dtype=torch.int64, device="cuda")


def leaf_enc(enc):
    """The encode() tuple with the entries the decoder reads as fresh leaves."""
    def leaf(t):
        return t.detach().clone().requires_grad_(True)
    return (leaf(enc[0]), None, (leaf(enc[2][0]), leaf(enc[2][1])), leaf(enc[3]), None, leaf(enc[5]),
            None, leaf(enc[7]), None, None)


def timed(fns, rounds, warm=1):
    ms = {k: [] for k in fns}
    for r in range(warm + rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warm:
                ms[k].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in ms.items()}


def peak_mib(model, fn):
    """Peak allocated memory of one call above the level before it, workspace caches dropped."""
    model.store.__dict__.pop("_order_grad_ws", None)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def routes(model, enc, orders):
    def run(score):
        def go():
            model.zero_grad()
            score(model.args, model, leaf_enc(enc), orders).sum().backward()
        return go
    return run(berson.score_orders_grad), run(berson.score_orders_autograd)


def part1(a):
    p = model_zoo.PRESETS["config3"]
    N = p["N"]
    m = model_zoo.build_preset("config3", device="cuda", dtype=torch.bfloat16, seed=0).train()
    data = bench.synthetic_batch(a.stories, N, p["per_seq"], 50265, 224, torch.device("cuda:0"),
                                 seed=2000)
    b = berson._batch_inputs(m, data)
    with torch.no_grad():
        enc = m.encode(**b)
    B, _N, H = enc[0].shape

    def encode():
        m.zero_grad()
        e = m.encode(**b)
        (e[0].sum() + e[3].sum() + e[5].sum() + e[7].sum() + e[2][0].sum()).backward()

    def full():
        m.zero_grad()
        m(data)[0].backward()

    out = []
    for K in (8, 32, 120):
        orders = orders_for(B, N, K, K)
        dev, auto = routes(m, enc, orders)
        ms = timed({"encode": encode, "device": dev, "autograd": auto, "full": full}, a.rounds)
        kc, nbytes = berson.K.order_grad_chunk(B, N, H, K, berson.SCORE_WS_CAP)
        out.append({"K": K, "a_encode_ms": round(ms["encode"], 3),
                    "b_device_ms": round(ms["device"], 3),
                    "b_share_of_encode": round(ms["device"] / ms["encode"], 4),
                    "c_autograd_ms": round(ms["autograd"], 3),
                    "c_over_b": round(ms["autograd"] / ms["device"], 2),
                    "d_full_pass_ms": round(ms["full"], 3),
                    "d_times_K_ms_extrapolated": round(ms["full"] * K, 1),
                    "b_candidates_per_call": int(kc), "b_workspace_mib": round(nbytes / 2 ** 20, 1),
                    "b_peak_mib": peak_mib(m, dev), "c_peak_mib": peak_mib(m, auto)})
    m.zero_grad()
    return {"N": N, "H": int(H), "stories": int(B), "by_K": out}


def part2(a):
    B, N, H, K = 8, 9, 1024, 64
    case = R.random_case(B, N, H, R.SEED)
    m = berson.BertForOrdering(berson.BersonConfig(hidden_size=H), model_zoo.berson_args(N, 60),
                               device="cuda", seed=1)
    m.load_state_dict({k: v for k, v in case["p"].items()}, strict=False)
    m.store.refresh_shadows()
    enc = (case["doc"].cuda(), None, (case["h0"][None].cuda(), case["c0"][None].cuda()),
           case["okey"].cuda(), None, case["cls_mat"].cuda(), None, case["cs_mat"].cuda(), None, None)
    orders = orders_for(B, N, K, 9)
    dev, auto = routes(m, enc, orders)
    ms = timed({"device": dev, "autograd": auto}, a.rounds)
    kc, nbytes = berson.K.order_grad_chunk(B, N, H, K, berson.SCORE_WS_CAP)
    return {"N": N, "H": H, "stories": B, "K": K, "b_device_ms": round(ms["device"], 3),
            "c_autograd_ms": round(ms["autograd"], 3),
            "c_over_b": round(ms["autograd"] / ms["device"], 2),
            "b_candidates_per_call": int(kc), "b_workspace_mib": round(nbytes / 2 ** 20, 1),
            "b_peak_mib": peak_mib(m, dev), "c_peak_mib": peak_mib(m, auto)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stories", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "order_grad_bench.log"))
    a = ap.parse_args()
    res = {"workload": "gradients of K candidate-order scores: mmseq_order_score_bwd vs the "
                       "torch-only route, beside the encode and K full passes (extrapolated)",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "config3": part1(a), "config5_head": part2(a)}
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
