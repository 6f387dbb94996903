#!/usr/bin/env python3
"""Headline benchmark: queries/sec of exact MoL top-k (BASELINE.json metric) on MI355X.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run does only what the headline needs: set-up, the W warm-up and K timed steps of the dense fp32 path and of the proved exact
path (the one `value` reports when it qualifies), the output dump, the JSON line.  --full adds everything else the line can carry, each
after the headline regions: the run without the seen-id filter, the f16x3 / f16-exact / f16x3-exact legs, the B = 1 / 8 and accuracy-protocol
matrix, the other workloads, the weight-scale sweep, the full-shard legs, the CPU baseline, HR parity against the CPU oracle chain, the
two-pass recall and coarse-scan roofline, and the sharded path's phase timings, pipelined rate and in-run checks.  The --no-* options
trim a --full run.

Workload (config.workload): amzn-books HSTU+MoL 8x8x32, N = 695 762 items, B = 32 queries per batch --
the configuration BASELINE.json's target is quoted on (">=10x the reference CPU queries/sec on amzn-books
8x8x32 MoL exact top-k at 1 GPU") and the largest of the real-dataset shapes; it fits one GPU.
One step = one pass of the hot path over one batch, the reference's timing protocol
(data/eval.py:128-170): CandidateIndex.get_top_k_outputs(k=120, truncate_k_prime_to=200) with the
seen-id filter on = query prologue -> fused MoL scoring of all N items -> exact top-200 -> id map ->
seen-id filter.  Inputs (item index, weights, queries, seen ids) are resident in HBM before the timed
region.  For N > 1 the corpus is sharded by item id (strong scaling: total N fixed) and the per-shard
top-k are merged after one RCCL all-gather.

Synthetic data: random-init weights with the reference's initialisers, counter-hash item table, LayerNorm'd
Gaussian queries; trained checkpoints / datasets are git-LFS pointers in the reference.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rails_amd  # noqa: E402
from rails_amd import engine as E  # noqa: E402
from rails_amd.sharded import ShardedMoLAvgTopK, ShardedMoLBruteForceTopK, shard_bounds  # noqa: E402

WORKLOADS = {
    # name: (oracle config key, N, seen-id width)
    "amzn-books": ("amzn-books", 695762, 61),
    "ml-20m": ("ml-20m", 27278, 211),
    "ml-1m": ("ml-1m", 3883, 211),
    # one 8-way shard of the synthetic configs of BASELINE.json (use --items to shrink)
    "synthetic-16x16x64": ("synthetic-16x16x64", 12_500_000, 0),
    "synthetic-8x8x32": ("synthetic-8x8x32", 125_000_000, 0),
}
PEAK_F32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_F16_MFMA_TFLOPS = 2500.0  # same guide: v_mfma_f32_32x32x16_f16, dense
# precision f16x3 issues three f16 MFMAs per algorithmic product block: its ceiling in algorithmic flops is a third of the f16 peak
PEAK_F16X3_TFLOPS = PEAK_F16_MFMA_TFLOPS / 3.0
PEAK_HBM_GBPS = 8000.0


VERIFIED = ("proved", "f16x3-exact", "f16-exact")   # modes whose output is the fp32 kernels' (first pass in split / plain f16, fp32 re-scoring)


def brute_force_module(mol, X, ids, precision: str):
    """MoLBruteForceTopK for a bench leg: "fp32" = the dense fp32 kernels (exact_mode "dense"), "proved" = the module's default exact path
    (split-f16 first pass under the a-priori bound, fp32 re-scoring: same bits), else the MoL module's opt-in precision of that name."""
    mol.precision = None if precision in ("fp32", "proved") else precision
    return rails_amd.MoLBruteForceTopK(mol, X, ids, exact_mode="proved" if precision == "proved" else "dense")


def flops_per_pair(cfg) -> int:
    """2*L*d (sub-embedding contraction) + 4*L*H (pair-gate MLP) + 12*L (combine/softmax/mix)."""
    L = cfg.query_dot_product_groups * cfg.item_dot_product_groups
    return 2 * L * cfg.dot_product_dimension + 4 * L * cfg.gating_qi_hidden_dim + 12 * L


def bytes_per_item_fp32(cfg) -> int:
    """fp32 index: (P_X*d + L) * 4 bytes per item, streamed once per batch."""
    L = cfg.query_dot_product_groups * cfg.item_dot_product_groups
    return (cfg.item_dot_product_groups * cfg.dot_product_dimension + L) * 4


def host_cpu_info() -> dict:
    """CPU model and physical core count of the box (the reference's protocol reports them, data/eval.py:139-170)."""
    model, phys = "unknown", set()
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                pid = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                cid = line.split(":", 1)[1].strip()
            elif not line.strip():
                if pid is not None and cid is not None:
                    phys.add((pid, cid))
                pid = cid = None
    except OSError:
        pass
    return {"cpu_model": model, "logical_cpus": os.cpu_count() or 1, "physical_cores": len(phys) or (os.cpu_count() or 1)}


def cpu_baseline(cfg, weights, q, user_ids, n_total: int, sample_items: int, k_prime: int):
    """The oracle (CPU restatement of the reference path, torch-CPU fp32, all host threads) on a bounded
    sample: all B queries against the first `sample_items` items, scaled linearly to N (the path is linear
    in N; top-k is <0.1 % of CPU time)."""
    from oracle import mol_oracle as O

    X = torch.from_numpy(O.hash_item_table(1, 0, sample_items, cfg.item_embedding_dim)).unsqueeze(0)
    ids = torch.arange(1, sample_items + 1, dtype=torch.int64).unsqueeze(0)
    B = q.shape[0]

    last = {}

    def run(n_items, chunk):
        t0 = time.perf_counter()
        last["out"] = O.brute_force_topk(cfg, weights, q, X[:, :n_items], ids[:, :n_items], min(k_prime, n_items), user_ids, chunk=chunk)
        return time.perf_counter() - t0

    # torch-CPU oversubscribes badly on many-core hosts (256 threads ran 30x slower than 8 here), so give the
    # baseline its best thread count: calibrate on a small slice, then time the bounded sample with the winner
    ncpu = os.cpu_count() or 1
    best = None
    for threads in sorted({t for t in (8, 16, 32, 64, 128, ncpu) if t <= ncpu}):
        torch.set_num_threads(threads)
        run(2048, 2048)  # warm-up at this thread count
        dt = run(4096, 4096)
        if best is None or dt < best[0]:
            best = (dt, threads)
    torch.set_num_threads(best[1])
    run(2048, 2048)
    dt = min(run(sample_items, 4096), run(sample_items, 4096))  # best of two passes: shared hosts are noisy
    qps = B / (dt * (n_total / sample_items))
    scaled = "" if sample_items == n_total else ", scaled linearly in N"
    return {
        "value": qps,
        "unit": "queries/s",
        "cores": torch.get_num_threads(),   # threads the timed passes actually used (the best of the calibration)
        "kind": "port",
        "sample": f"B={B} queries x {'all' if sample_items == n_total else 'first'} {sample_items} of {n_total} items, best of 2 timed passes ({dt:.1f} s each) at the best of 8..{ncpu} threads{scaled}",
        **host_cpu_info(),
        # the oracle's own (scores, 1-based item ids) of the last timed pass when it covered the whole corpus: hr_parity re-uses it (not part of the JSON line)
        "_oracle_topk": last["out"][:2] if sample_items == n_total else None,
    }


def measurement_matrix(mol, X, ids, q, kw, inv, cfg, n_items: int, steps: int, dev) -> list:
    """Points of the reference's timing protocol (data/eval.py:128-170) beside the headline one, same step definition
    (get_top_k_outputs), both precisions and the verified fast mode: (B, k, k') = (1, 120, 200), (8, 120, 200) and the accuracy protocol (32, 2500, 2561)."""
    points = []
    for precision in ("fp32", "proved", "f16x3", "f16-exact"):
        with torch.inference_mode():
            tk = brute_force_module(mol, X, ids, precision)
            cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
            for Bx, kx, trunc in ((1, 120, 200), (8, 120, 200), (q.shape[0], 2500, None)):
                qx, invx = q[:Bx], inv[:Bx]
                kwx = {key: v[:Bx] for key, v in kw.items()}
                kx = min(kx, n_items)
                for _ in range(2):
                    cand.get_top_k_outputs(qx, kx, kwx, tk, invx, truncate_k_prime_to=trunc)
                torch.cuda.synchronize()
                t_est = time.perf_counter()
                for _ in range(3):
                    cand.get_top_k_outputs(qx, kx, kwx, tk, invx, truncate_k_prime_to=trunc)
                torch.cuda.synchronize()
                t_est = (time.perf_counter() - t_est) / 3
                # ~30 ms of the same calls right before each timed region: the f16 kernels lose their clocks within milliseconds of idle and
                # need ~20 ms of load to get them back (tools/r05_ramp_probe.py); these legs are shorter than that at small batches
                n_warm = max(2, min(64, int(0.03 / max(t_est, 1e-5)) + 1))
                dt, per = float("inf"), None
                for _ in range(2):   # secondary points: the better of two timed regions (one-off stalls of 20-70 ms -- one step of one leg -- were seen in three runs out of three)
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
                    for _ in range(n_warm):
                        cand.get_top_k_outputs(qx, kx, kwx, tk, invx, truncate_k_prime_to=trunc)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(steps):
                        ev[i].record()
                        cand.get_top_k_outputs(qx, kx, kwx, tk, invx, truncate_k_prime_to=trunc)
                    ev[steps].record()
                    torch.cuda.synchronize()
                    d_ = (time.perf_counter() - t0) / steps
                    if d_ < dt:
                        dt, per = d_, torch.tensor([ev[i].elapsed_time(ev[i + 1]) for i in range(steps)])
                eng = tk._bind()
                qp, _, _ = eng.query_pack(qx, kwx.get("user_ids"))
                buf = torch.empty((Bx, n_items), dtype=torch.float32, device=dev)
                eng.score_dense(qp, Bx, tk._index, out=buf)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    eng.score_dense(qp, Bx, tk._index, out=buf)
                e1.record()
                torch.cuda.synchronize()
                kms = e0.elapsed_time(e1) / steps
                tf = Bx * n_items * flops_per_pair(cfg) / (kms * 1e-3) / 1e12
                if precision in VERIFIED:    # output = the fp32 path's; the first pass is not a parity kernel: no roofline fractions
                    st = tk.stats()
                    points.append({
                        "precision": precision, "batch": Bx, "k": kx, "k_prime": min(kx + inv.shape[1], n_items) if trunc is None else min(trunc, n_items),
                        "queries_per_s": Bx / dt, "ms_per_step": dt * 1e3, "ms_per_step_stdev": float(per.std()) if steps > 1 else 0.0,
                        "first_pass_kernel_ms": kms, "rescore_calls": st["calls"], "dense_fp32_fallbacks": st["fallbacks"],
                        **({"proved_calls": st.get("proved_calls", 0), "eps_a_priori": st.get("eps_rigorous")} if precision == "proved" else {}),
                    })
                    continue
                points.append({
                    "precision": precision, "batch": Bx, "k": kx, "k_prime": min(kx + inv.shape[1], n_items) if trunc is None else min(trunc, n_items),
                    "queries_per_s": Bx / dt, "ms_per_step": dt * 1e3, "ms_per_step_stdev": float(per.std()) if steps > 1 else 0.0,
                    "scoring_kernel_ms": kms, "scoring_tflops_algorithmic": tf,
                    "mfma_frac": tf / (PEAK_F32_MFMA_TFLOPS if precision == "fp32" else PEAK_F16X3_TFLOPS),
                    "hbm_frac": n_items * bytes_per_item_fp32(cfg) / (kms * 1e-3) / 1e9 / PEAK_HBM_GBPS,
                })
            del tk
    mol.precision = None
    return points


def committed_traffic(key: str):
    """HBM bytes per launch of a scoring kernel from the committed PMC passes (profiles/pmc_summary.json; not collected in the run)."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "pmc_summary.json"))).get(key)
        return rec and rec.get("hbm_bytes_per_launch")
    except Exception:
        return None


def quick_workload(name: str, B: int, k: int, kp: int, steps: int, dev, items: int = 0, precision: str = "fp32") -> dict:
    """Secondary measurement of another BASELINE.json config on one GPU (same step definition, fewer steps)."""
    from oracle import mol_oracle as O

    cfg_key, N, width = WORKLOADS[name]
    N = items or N
    cfg = O.CONFIGS[cfg_key]
    weights = O.synthetic_weights(cfg, seed=0)
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
        cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
        cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
        query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None)
    mol.load_state_dict(weights, strict=True)
    mol = mol.to(dev).eval()
    X = torch.from_numpy(O.hash_item_table(1, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B).to(dev)
    kw = {}
    if len(cfg.uid_embedding_hash_sizes) > 0:
        g = torch.Generator().manual_seed(3)
        kw["user_ids"] = torch.randint(0, cfg.uid_embedding_hash_sizes[0], (B,), generator=g, dtype=torch.int64).to(dev)
    with torch.inference_mode():
        tk = brute_force_module(mol, X, ids, precision)
        cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
        _, top_ids = tk(q, k=min(kp, N), **kw)
        inv = torch.zeros((B, max(width, 1)), dtype=torch.int64, device=dev)
        g = torch.Generator().manual_seed(4)
        for b in range(B):
            sel = torch.randperm(top_ids.shape[1], generator=g)[: width // 2].to(dev)
            inv[b, : width // 2] = top_ids[b, sel]
        for _ in range(3):
            cand.get_top_k_outputs(q, k, kw, tk, inv, truncate_k_prime_to=kp)
        dt = float("inf")
        for _ in range(2):   # secondary legs: the better of two timed regions (a one-off host stall of ~0.2 s was seen once in one region)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                cand.get_top_k_outputs(q, k, kw, tk, inv, truncate_k_prime_to=kp)
            torch.cuda.synchronize()
            dt = min(dt, (time.perf_counter() - t0) / steps)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        def dominant():     # prologue + the scoring launch that dominates the step (the split-f16 first pass of a verified mode)
            eng_ = tk._bind()
            if eng_.exact is not None:
                qp_, _, _ = eng_.query_pack(q, kw.get("user_ids"))
                return eng_.score_dense(qp_, B, tk._index)
            return tk.all_logits(q, **kw)
        dominant()
        e0.record()
        for _ in range(steps):
            dominant()
        e1.record()
        torch.cuda.synchronize()
        score_ms = e0.elapsed_time(e1) / steps   # prologue + scoring kernel
        # Small corpora: the eager step is 4 launches of 5-30 us each -- on a box whose host CPUs are busy it becomes host-bound
        # (seen: 61 us on an idle host, 210-250 us on a loaded one, same GPU work).  The same step replayed from a captured hipGraph
        # (the path has no host sync and no allocation-dependent control flow) is the host-independent figure; reported beside the
        # eager one, with the replay's output compared bit for bit.
        graph = {}
        if N <= 100_000 and precision not in VERIFIED:
            try:
                ref_i, ref_s, _ = cand.get_top_k_outputs(q, k, kw, tk, inv, truncate_k_prime_to=kp)
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(3):
                        cand.get_top_k_outputs(q, k, kw, tk, inv, truncate_k_prime_to=kp)
                torch.cuda.current_stream(dev).wait_stream(side)
                g_ = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_):
                    gi, gs, _ = cand.get_top_k_outputs(q, k, kw, tk, inv, truncate_k_prime_to=kp)
                g_.replay()
                torch.cuda.synchronize()
                same = bool(torch.equal(gi, ref_i) and torch.equal(gs, ref_s))
                gdt = float("inf")
                for _ in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps * 5):
                        g_.replay()
                    torch.cuda.synchronize()
                    gdt = min(gdt, (time.perf_counter() - t0) / (steps * 5))
                graph = {"graph_replay_ms_per_step": gdt * 1e3, "graph_replay_output_identical": same}
                del g_
            except Exception as e:   # noqa: BLE001 -- a secondary figure must not take the leg down
                graph = {"graph_replay_error": f"{type(e).__name__}: {e}"[:200]}
    tf = B * N * flops_per_pair(cfg) / (score_ms * 1e-3) / 1e12
    traffic = None
    if name == "synthetic-16x16x64" and N == 400_000 and B == 32:
        traffic = committed_traffic("synthetic-16x16x64:N400k:B32:r03:" + {"fp32": "fp32", "f16x3": "f16x3", "f16-exact": "f16x1"}.get(precision, precision))
    tr = {"traffic": traffic, "traffic_source": "profiles/pmc_summary.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the scoring kernel on this workload; FETCH_SIZE x 2 on gfx950; not collected in this run)",
          "hbm_bytes_alg_per_launch": N * bytes_per_item_fp32(cfg) + B * N * 4} if traffic else {}
    if precision in VERIFIED:   # verified fast mode: output identical to fp32 (tests); the first pass is not a parity kernel, no roofline claim
        st = tk.stats()
        return {"workload": f"{name} {cfg.query_dot_product_groups}x{cfg.item_dot_product_groups}x{cfg.dot_product_dimension}, N={N}", "precision": precision,
                "queries_per_s": B / dt, "ms_per_step": dt * 1e3, "prologue_plus_first_pass_ms": score_ms,
                "rescore_calls": st["calls"], "dense_fp32_fallbacks": st["fallbacks"],
                **({"proved_calls": st.get("proved_calls", 0), "eps_a_priori": st.get("eps_rigorous"),
                    "runs_dense_fp32": tk._bind().exact is None, "bound": st.get("bound_kind", "one a-priori eps")} if precision == "proved" else {}), **tr}
    return {"workload": f"{name} {cfg.query_dot_product_groups}x{cfg.item_dot_product_groups}x{cfg.dot_product_dimension}, N={N}", "precision": precision,
            "queries_per_s": B / dt, "ms_per_step": dt * 1e3, "prologue_plus_scoring_ms": score_ms, **graph,
            "scoring_tflops_algorithmic_lower_bound": tf,
            "mfma_frac_lower_bound": tf / (PEAK_F32_MFMA_TFLOPS if precision == "fp32" else PEAK_F16X3_TFLOPS), **tr}


def weights_scale_sweep(cfg, weights, X, ids, q, kw, inv, k: int, kp: int, steps: int, dev, scales=(1.0, 1.5, 2.0, 3.0, 4.0)) -> list:
    """Where a model lands on the proved mode's provability cliff (round-5 review, weak 2): the a-priori bound grows quadratically with the
    pair-gate weight scale, so a trained checkpoint with heavier gates than random init may get the per-pair form of the bound, or -- beyond
    PROVED_MAX_EPS_PER_PAIR -- the dense fp32 kernels.  Per scale s (both pair-gate weight matrices x s): the bound's eps at |cl| <= 1/tau,
    the form the module binds (one eps / per-pair upper bound / dense), proved and fallback counts over the timed steps, queries/s; the output
    is checked against the dense fp32 kernels' on the same weights."""
    p = "_gating_fn._qi_partial_module."
    rows = []
    for sc in scales:
        w = dict(weights)
        w[p + "1.weight"] = weights[p + "1.weight"] * sc
        w[p + "3.weight"] = weights[p + "3.weight"] * sc
        mol, _ = rails_amd.create_mol_interaction_module(
            cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
            cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
            cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
            query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None)
        mol.load_state_dict(w, strict=True)
        mol = mol.to(dev).eval()
        with torch.inference_mode():
            tk = rails_amd.MoLBruteForceTopK(mol, X, ids, exact_mode="proved")      # (bench sets the class default to "dense" for its hand-driven legs)
            dense = rails_amd.MoLBruteForceTopK(mol, X, ids, exact_mode="dense")
            cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
            ref = cand.get_top_k_outputs(q, k, kw, dense, inv, truncate_k_prime_to=kp)
            del dense
            for _ in range(3):
                out = cand.get_top_k_outputs(q, k, kw, tk, inv, truncate_k_prime_to=kp)
            same = bool(torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]))
            st0 = tk.stats() if tk._bind().exact is not None else {}
            torch.cuda.synchronize()
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]      # per-step device time; the median is immune to a one-off host stall
            evs[0].record()
            for j in range(steps):
                cand.get_top_k_outputs(q, k, kw, tk, inv, truncate_k_prime_to=kp)
                evs[j + 1].record()
            torch.cuda.synchronize()
            per = sorted(evs[j].elapsed_time(evs[j + 1]) for j in range(steps))
            dt = per[len(per) // 2] * 1e-3
            bound = tk._bound_from_weights(tk._mol_module.engine().spec)
            binds = tk._bind().exact is not None
            st = tk.stats() if binds else {}
            rows.append({"pair_gate_weight_scale": sc, "eps_at_max_abs_cl": float(bound.get("eps", float("inf"))),
                         "route": ("proved, " + st.get("bound_kind", "one a-priori eps")) if binds else "dense fp32 kernels (bound beyond PROVED_MAX_EPS_PER_PAIR or no UPPER build)",
                         "candidates_per_query": st.get("kc"), "timed_calls": steps,
                         "proved_calls": st.get("proved_calls", 0) - st0.get("proved_calls", 0), "dense_fp32_fallbacks": st.get("fallbacks", 0) - st0.get("fallbacks", 0),
                         "bound_violations": st.get("bound_violations", 0), "queries_per_s": q.shape[0] / dt, "ms_per_step": dt * 1e3, "timing": "median over the timed steps, device events",
                         "output_identical_to_fp32_path": same})
        del tk, mol
        torch.cuda.empty_cache()
    return rows


def hr_parity_leg(cfg, weights, mol, B: int, k: int, kp: int, dev, n_items: int = 65_536, shared=None, exact_mode: str = "dense") -> dict:
    """The quality half of BASELINE.json's metric ("queries/sec + HR@10/50 parity"): HR@k / NDCG@10 / MRR of the HIP path against the
    CPU oracle chain on the same inputs -- seen ids taken from each row's own winners, and targets PLANTED at known oracle ranks
    (uniform in 1..100, absent for ~15 % of the rows) so that the metrics are not trivially 0 or 1 (trained checkpoints are git-LFS
    pointers: SURVEY.md section 2).  Both sides run the reference's harness arithmetic (data/eval.py:194-243: rank of the target in the
    returned ids, HR@k = rank <= k, NDCG@k, MRR) on their OWN returned ids; the GPU side goes through rails_amd.eval_harness
    (get_eval_state + eval_metrics_v2_from_tensors, the reference's protocol incl. its k / k' / truncate rules).
    shared = (q, user_ids, N, (oracle scores, oracle 1-based positions)): the HEADLINE corpus (table seed 1, all N items) and the oracle pass the
    cpu_baseline leg has just timed over it -- one oracle pass serves both legs; without it a 65 536-item sub-corpus of the workload's shape
    is scored by the oracle here.  Not timed; runs after the headline region."""
    from oracle import mol_oracle as O
    from rails_amd import eval_harness as H

    g = torch.Generator().manual_seed(6)
    width = 40
    if shared is not None:
        q, uid, N, (rs, rpos) = shared
        X = torch.from_numpy(O.hash_item_table(1, 0, N, cfg.item_embedding_dim)).unsqueeze(0)
        ids = (torch.arange(N, dtype=torch.int64) * 3 + 7).unsqueeze(0)      # sparse ids, as the datasets have
        ri = (rpos - 1) * 3 + 7                                                # the oracle pass numbered the items 1..N
        oracle_s = None
        seen = torch.zeros((B, width), dtype=torch.int64)
        kpr = O.k_prime(k, seen, N, kp)                                        # the harness's k' for this width (160); the shared pass is sorted: its prefix is the top-k'
        assert rs.shape[1] >= kpr, "the shared oracle pass must have selected at least k' candidates"
        rs, ri = rs[:, :kpr], ri[:, :kpr]
    else:
        N = n_items
        X = torch.from_numpy(O.hash_item_table(2, 0, N, cfg.item_embedding_dim)).unsqueeze(0)
        ids = (torch.arange(N, dtype=torch.int64) * 3 + 7).unsqueeze(0)
        q = O.synthetic_queries(cfg, B, seed=5)
        uid = torch.randint(0, 5000, (B,), generator=g) if len(cfg.uid_embedding_hash_sizes) else None
        seen = torch.zeros((B, width), dtype=torch.int64)
        t0 = time.perf_counter()
        rs, ri, _ = O.brute_force_topk(cfg, weights, q, X, ids, O.k_prime(k, seen, N, kp), uid)
        oracle_s = time.perf_counter() - t0
    for b in range(B):   # 20 of each row's own top-60, so that the filter really removes winners
        seen[b, :20] = ri[b, torch.randperm(60, generator=g)[:20]]
    ref_ids, ref_sc = O.filter_seen_ids(ri, rs, seen, k)
    planted = torch.randint(0, 100, (B,), generator=g)
    target = ref_ids[torch.arange(B), planted].clone()
    target[torch.rand(B, generator=g) < 0.15] = ids[0, -1]   # an id that is practically never retrieved
    target = target.unsqueeze(1)
    ref = O.eval_metrics(ref_ids, target, k)

    class Enc:      # the encoder is upstream of the path: replay the query embeddings
        def encode(self, **kw):
            return q.to(dev)

        def get_item_embeddings(self, item_ids):
            return X.to(dev)[0][(item_ids.to(dev) - 7) // 3]

    model = Enc()
    model._ndp_module = mol
    feats = H.SequentialFeatures(torch.full((B,), width), seen.to(dev), None, {"user_ids": uid.to(dev)} if uid is not None else {})
    with torch.inference_mode():
        state = H.get_eval_state(model, ids[0].tolist(), None, lambda e, i: rails_amd.MoLBruteForceTopK(mol, e, i, exact_mode=exact_mode), dev)
        got = H.eval_metrics_v2_from_tensors(state, model, feats, target.to(dev), include_eval_time=True, include_eval_top_k_ids=True)
    got_ids = got["eval_top_k_ids"].cpu()
    out = {"what": f"HIP path ({'proved exact path' if exact_mode == 'proved' else 'dense fp32 kernels'}) vs CPU oracle chain, "
                   f"{'the headline corpus: all ' if shared is not None else ''}{N} items of the workload's shape, B = {B}, k = {k}, k' = {kp} (timing protocol), 20 seen ids per row, "
                   "targets planted at oracle ranks 1..100 (15 % absent)" + ("; the oracle pass is the one cpu_baseline timed" if shared is not None else ""),
           "identical_rows": int((got_ids == ref_ids).all(1).sum()), "rows": B,
           "ids_identical_fraction": float((got_ids == ref_ids).float().mean()), "oracle_cpu_seconds": oracle_s}
    for key in ("hr@1", "hr@5", "hr@10", "hr@50", "hr@100", "ndcg@10", "mrr"):
        mine, theirs = got[key].float().cpu(), ref[key].float()
        out[key] = {"hip": float(mine.mean()), "oracle": float(theirs.mean()), "rows_differing": int(((mine - theirs).abs() > 1e-6).sum())}
    # rows whose ids differ from the oracle's: only swaps inside groups of ORACLE scores closer than the two paths' rounding (2e-5; SURVEY.md
    # section 7 "bit-exact indices vs ties") -- same id set, and at every differing position the oracle's scores of the two ids are that close
    tie_rows = 0
    for b in range(B):
        if bool((got_ids[b] == ref_ids[b]).all()):
            continue
        pos_of = {int(v): j for j, v in enumerate(ref_ids[b].tolist())}
        diff = (got_ids[b] != ref_ids[b]).nonzero().flatten().tolist()
        if set(got_ids[b].tolist()) == set(pos_of) and all(abs(float(ref_sc[b, j]) - float(ref_sc[b, pos_of[int(got_ids[b, j])]])) <= 2e-5 for j in diff):
            tie_rows += 1
    out["rows_differing_only_inside_oracle_ties"] = tie_rows
    out["parity"] = bool(out["identical_rows"] + tie_rows == B and all(out[key]["rows_differing"] == 0 for key in ("hr@1", "hr@5", "hr@10", "hr@50", "hr@100", "ndcg@10", "mrr")))
    return out


PLANTED_GATE_KEYS = ("_gating_fn._query_only_partial_module.2.weight", "_gating_fn._item_only_partial_module.3.weight",
                     "_gating_fn._qi_partial_module.3.weight", "_gating_fn._qi_partial_module.3.bias")


def planted_weights(weights: dict, gate_scale: float = 0.25) -> dict:
    """Random-init MoL weights with the gate networks' output layers scaled down: near-uniform mixture weights, so that MoL ~ the
    coarse dot product + a gate perturbation and a two-pass search has structure to find.  (At the reference's plain random init the
    coarse score of pass 1 is uncorrelated with the MoL logit and recall is ~ K'/N whatever the implementation.)"""
    w = dict(weights)
    for key in PLANTED_GATE_KEYS:
        w[key] = w[key] * gate_scale
    return w


def two_pass_recall(at, q, k: int, chunk: int = 8) -> dict:
    """recall@10 / recall@k of a two-pass module (MoLAvgTopK semantics: coarse top-K' + MoL rerank, rails/indexing/mol_top_k.py:328-396)
    against EXACT brute force over the same shard: the exact side scores every item with the module's own fp32 kernels (`chunk`
    queries = chunk * N * 4 bytes of logits at a time) and selects with the exact top-k."""
    _, got = at(q, k=k)
    hits10 = hitsk = 0
    B = q.shape[0]
    for b0 in range(0, B, chunk):
        logits = at.all_logits(q[b0 : b0 + chunk])
        _, truth = E.topk(logits, k, ids=at._ids_flat)
        del logits
        for r in range(truth.shape[0]):
            mine, ref = got[b0 + r].tolist(), truth[r].tolist()
            hits10 += len(set(mine[:10]) & set(ref[:10]))
            hitsk += len(set(mine) & set(ref))
    return {"recall@10": hits10 / (B * 10), f"recall@{k}": hitsk / (B * k), "k": k, "queries": B,
            "against": "exact brute-force MoL top-k over the same items (fp32 kernels, every item scored)"}


def full_shard_legs(B: int, k: int, dev) -> list:
    """BASELINE.json configs 4 and 5 at the size of ONE 8-way shard on this GPU (12.5 M items of 16x16x64, exact top-k in three precisions;
    125 M items of 8x8x32, two-pass MoLAvgTopK with K' = 1000): what each of the 8 ranks of `--gpus 8 --workload synthetic-*` runs before the
    all-gather, timed through the module API.  Item tables drawn on the device by the counter hash (rails_hash_item_table).  A leg is skipped, and says so,
    when the device lacks the memory for it (config 5 needs ~210 GB: 32 GB table + 160 GB index + 8 GB coarse table + buffers)."""
    import gc
    from oracle import mol_oracle as O

    def build(cfg_key, n, precision):
        cfg = O.CONFIGS[cfg_key]
        mol, _ = rails_amd.create_mol_interaction_module(
            cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
            cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
            cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
            query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None)
        mol.load_state_dict(O.synthetic_weights(cfg, seed=0), strict=True)
        mol = mol.to(dev).eval()
        mol.precision = None if precision in ("fp32", "proved") else precision
        X = E.hash_item_table(1, 0, n, cfg.item_embedding_dim, dev).unsqueeze(0)   # counter hash, drawn on the device (reproducible on a CPU by id)
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).unsqueeze(0)
        return cfg, mol, X, ids, O.synthetic_queries(cfg, B).to(dev)

    def timed(fn, warm, steps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    legs = []
    for name, n, need_gb, variants in (("synthetic-16x16x64", 12_500_000, 150, ("fp32", "proved", "f16x3", "f16-exact")), ("synthetic-8x8x32", 125_000_000, 235, ("two-pass",))):
        for variant in variants:
            gc.collect()
            torch.cuda.empty_cache()
            free = torch.cuda.mem_get_info(dev)[0]
            label = {"workload": f"{name}, one 8-way shard, N={n}", "batch": B, "k": k}
            if free < need_gb * 1e9:
                legs.append({**label, "variant": variant, "skipped": f"needs {need_gb} GB of free device memory, {free / 1e9:.0f} GB available"})
                continue
            with torch.inference_mode():
                cfg, mol, X, ids, q = build(name, n, "fp32" if variant == "two-pass" else variant)
                cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
                t0 = time.perf_counter()
                if variant == "two-pass":
                    mod = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=1000)
                    mod._table()
                else:
                    mod = rails_amd.MoLBruteForceTopK(mol, X, ids, exact_mode="proved" if variant == "proved" else "dense")
                    mod._bind()
                torch.cuda.synchronize()
                build_s = time.perf_counter() - t0
                dt = timed(lambda: cand.get_top_k_outputs(q, k, {}, mod, None), 2, 10 if variant == "two-pass" else 3)
                leg = {**label, "variant": variant if variant != "two-pass" else "two-pass MoLAvgTopK, K'=1000 (coarse bf16 scan + MoL rerank)", "queries_per_s": B / dt,
                       "ms_per_step": dt * 1e3, "index_build_s": build_s, "item_table": "device counter hash"}
                if variant == "two-pass":
                    # the same calls with batch i + 1 submitted before batch i's verdict word is read (MoLAvgTopK.submit / result)
                    def pipelined(n, depth=2):     # two batches submitted ahead of the one whose result is taken
                        hs = [mod.submit(q, k) for _ in range(min(depth, n))]
                        submitted = len(hs)
                        for i in range(n):
                            if submitted < n:
                                hs.append(mod.submit(q, k))
                                submitted += 1
                            out = mod.result(hs.pop(0))
                        return out
                    p_out = pipelined(2)
                    r_ids, r_scores, _ = cand.get_top_k_outputs(q, k, {}, mod, None)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pipelined(10)
                    torch.cuda.synchronize()
                    dtp = (time.perf_counter() - t0) / 10
                    leg["pipelined"] = {"ms_per_step": dtp * 1e3, "queries_per_s": B / dtp, "hbm_frac_lower_bound": int(mod._prefilter(count=False).numel() if mod._prefilter(count=False) is not None else mod._table().numel() * mod._table().element_size()) / dtp / 8.0e12,
                                        "output_equal_to_unpipelined": bool(torch.equal(p_out[0], r_scores) and torch.equal(p_out[1], r_ids))}
                    leg["coarse_table_bytes"] = int(mod._table().numel() * mod._table().element_size())
                    leg["int8_prefilter_bytes"] = int(mod._prefilter(count=False).numel()) if mod._prefilter(count=False) is not None else 0
                    # the whole step (prologue, sample + threshold, select scan, key selection, in-place rerank, final top-k) against ONE read of the table
                    leg["hbm_frac_lower_bound"] = (leg["int8_prefilter_bytes"] or leg["coarse_table_bytes"]) / dt / 8.0e12   # the bytes the streaming pass reads once
                    # north_star: "recall@k vs exact reported".  On the planted-structure weights (the plain random init has nothing
                    # for a two-pass search to find): the module is rebuilt on the same table -- one 160 GB index at a time
                    del mod, cand
                    torch.cuda.empty_cache()
                    w_p = planted_weights(O.synthetic_weights(cfg, seed=0))
                    mol.load_state_dict({kk: vv.to(dev) if torch.is_tensor(vv) else vv for kk, vv in w_p.items()}, strict=True)
                    mod = rails_amd.MoLAvgTopK(mol, X, ids, avg_top_k=1000)
                    leg["recall"] = {**two_pass_recall(mod, q, k), "avg_top_k": 1000, "weights": "planted structure: gate output layers x 0.25"}
                    cand = None
                elif variant == "fp32" or variant == "f16x3":
                    tf = B * n * flops_per_pair(cfg) / dt / 1e12       # lower bound: the step also holds the prologue and the selection
                    leg["tflops_algorithmic_lower_bound"] = tf
                    leg["mfma_frac_lower_bound"] = tf / (PEAK_F32_MFMA_TFLOPS if variant == "fp32" else PEAK_F16X3_TFLOPS)
                else:
                    st = mod.stats()
                    leg["rescore_calls"], leg["dense_fp32_fallbacks"] = st["calls"], st["fallbacks"]
                    if variant == "proved":
                        leg["proved_calls"], leg["eps_a_priori"], leg["candidates_per_query"] = st.get("proved_calls", 0), st.get("eps_rigorous"), st.get("kc")
                        leg["runs_dense_fp32"] = mod._bind().exact is None
                        leg["bound"] = st.get("bound_kind", "one a-priori eps")
                        leg["bound_violations"] = st.get("bound_violations", 0)
                        if st.get("upper_bound_poly") is not None:
                            leg["upper_bound_poly"] = st["upper_bound_poly"]
                legs.append(leg)
                del mod, cand, X, ids, mol
    gc.collect()
    torch.cuda.empty_cache()
    return legs


DUMP_MAX_BYTES = 64 << 20


def host_copy(outputs):
    """(top_k_ids, top_k_scores) of a step as host tensors: taken after the timed region, before later calls can reuse the buffers."""
    return tuple(t.detach().to("cpu", copy=True) for t in outputs)


def dump_outputs(dirname: str, arrays: dict) -> dict:
    """--dump-outputs: every (rows, ...) tensor of `arrays` as dirname/<name>.npy -- integers as float64 (exact below 2^53), floats as
    float32 (float64 stays float64).  Above DUMP_MAX_BYTES in all, the same fixed seeded sample of rows is kept of every array, its row
    indices written beside them as rows.npy."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    host = {name: t.to(torch.float64 if (t.dtype == torch.float64 or not t.is_floating_point()) else torch.float32).numpy()
            for name, t in arrays.items()}
    n_rows = next(iter(host.values())).shape[0]
    row_bytes = sum(a.nbytes for a in host.values()) // max(n_rows, 1)
    budget = DUMP_MAX_BYTES - 1024     # room for the .npy headers
    sampled = row_bytes * n_rows > budget
    if sampled:
        keep = max(1, budget // (row_bytes + 8))
        rows = torch.randperm(n_rows, generator=torch.Generator().manual_seed(0))[:keep].sort().values.numpy()
        host = {name: a[rows] for name, a in host.items()}
        host["rows"] = rows.astype(np.float64)
    for name, a in host.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    return {"dir": dirname, "files": {name + ".npy": [list(a.shape), str(a.dtype)] for name, a in host.items()}, "sampled_rows": bool(sampled)}


def main() -> None:
    # The cyclic garbage collector stays off while anything is timed: a generation-2 collection of this process (torch modules, numpy
    # fixtures, thousands of event objects) is a 30-40 ms host pause, and a step is 2-6 ms -- one collection inside a 20-step region
    # reads as + 2 ms per step (seen as 4.7 instead of 2.8 ms on the f16x3-exact leg; the kernel trace showed the GPU idle for 30.6 ms
    # in front of ONE launch).  Reference counting still frees every tensor at once; cycles are collected between the legs.
    import gc

    gc.disable()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="amzn-books", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--k", type=int, default=120)
    ap.add_argument("--k-prime", type=int, default=200)
    ap.add_argument("--cpu-sample-items", type=int, default=0, help="items of the CPU-baseline sample (0 = the whole corpus: ~10 s per pass on a many-core host)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-fast-path", action="store_true", help="skip the extra f16x3 measurement")
    ap.add_argument("--no-other-workloads", action="store_true", help="skip the secondary ML-20M / ML-1M measurements")
    ap.add_argument("--no-matrix", action="store_true", help="skip the B = 1 / 8 and accuracy-protocol points")
    ap.add_argument("--no-recall", action="store_true", help="--two-pass: skip the recall@k measurement against exact brute force (planted-structure weights)")
    ap.add_argument("--no-hr-parity", action="store_true", help="skip the HR@k / NDCG / MRR comparison with the CPU oracle chain (the metric's quality half)")
    ap.add_argument("--no-weights-sweep", action="store_true", help="skip the pair-gate weight-scale sweep of the proved mode (eps, route, proved / fallback counts per scale)")
    ap.add_argument("--no-full-shards", action="store_true", help="skip the legs that run one full 8-way shard of BASELINE configs 4 and 5 (12.5 M / 125 M items) on this GPU")
    ap.add_argument("--items", type=int, default=0, help="override the workload's corpus size N (total over all ranks)")
    ap.add_argument("--device-table", action="store_true",
                    help="draw the item table on the GPU (the same counter hash, rails_hash_item_table) instead of on the host; "
                         "implied above 4 M items per rank (a 125 M-item shard is 32 GB)")
    ap.add_argument("--two-pass", type=int, default=0, metavar="K'",
                    help="BASELINE config 5: MoLAvgTopK(K' per shard) = fused coarse top-K' + MoL rerank, instead of exact "
                         "brute force (the default, and the only mode the headline metric is quoted on)")
    ap.add_argument("--precision", default="proved", choices=["proved", "fp32-dense"],
                    help="exact brute force: 'proved' (default) = the module's default exact path -- split-f16 first pass under the a-priori error bound, "
                         "fp32 re-scoring of the candidates, device-side proof per call; the fp32 kernels' bits -- reported as `value` when every timed call "
                         "was proved and the output is identical to the dense fp32 path's (else, and with 'fp32-dense', `value` = the dense fp32 kernels)")
    ap.add_argument("--pipeline", action="store_true",
                    help="N > 1: time the steps with batch i's all-gather + merge + filter overlapped with batch i+1's prologue + scoring "
                         "(ShardedTopK.submit / result, two streams); without it, --full still reports the pipelined rate next to `value`")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the run, write what the path reported as `value` returned in its last timed step (top_k_ids as float64, "
                         "top_k_scores as float32) to DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every secondary measurement and check (see the module docstring); a plain run times "
                         "the headline alone.  The --no-* options trim a --full run")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: launch torch.distributed.run with one rank per GPU and the same argv as a fresh child process
        import socket
        import subprocess

        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        rc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
                             "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]).returncode
        sys.exit(rc)

    from oracle import mol_oracle as O  # inputs generator + cpu_baseline checker only

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    # RAILS_BENCH_TEST_BACKEND=gloo is a TEST hook: several ranks share GPU 0 and the (tiny) all-gather message is
    # staged through the host, so the sharded code path can be exercised on a one-GPU box.  Never set by the driver.
    test_backend = os.environ.get("RAILS_BENCH_TEST_BACKEND")
    # RAILS_BENCH_TEST_ONE_RANK_EXCHANGE=1 is a TEST hook too: with --gpus 1 the run takes the SHARDED path in a process group of one rank over
    # backend nccl -- a one-GPU box cannot hold two RCCL ranks, but this way RCCL's all-gather / all-reduce / barrier on device tensors, the
    # exchange stream and the merge launches all execute once on the part before the driver's multi-GPU run.  Never set by the driver.
    one_rank_exchange = world == 1 and bool(os.environ.get("RAILS_BENCH_TEST_ONE_RANK_EXCHANGE"))
    sharded = world > 1 or one_rank_exchange
    if one_rank_exchange:
        from rails_amd.sharded import ShardedTopK

        ShardedTopK.EXCHANGE_WITH_ONE_RANK = True
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if test_backend:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if sharded:
        import torch.distributed as dist

        import datetime

        # a hung collective must end the run with rc != 0, not with a number: asynchronous errors tear the process down after
        # RAILS_BENCH_COLLECTIVE_TIMEOUT_S (default 120 s: the first collective includes RCCL's communicator set-up over xGMI)
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
        coll_timeout = datetime.timedelta(seconds=int(os.environ.get("RAILS_BENCH_COLLECTIVE_TIMEOUT_S", "120")))
        if test_backend:
            dist.init_process_group(test_backend, timeout=coll_timeout)
        else:
            if torch.cuda.device_count() < world:
                raise SystemExit(f"--gpus {world} needs {world} visible devices, found {torch.cuda.device_count()} (one rank per GPU over RCCL)")
            dist.init_process_group("nccl", device_id=dev, timeout=coll_timeout)
            if dist.get_backend() != "nccl":
                raise SystemExit(f"backend is {dist.get_backend()}, expected nccl (= RCCL on ROCm)")

    def all_gather_rows(msg):
        """(B, W) -> (world * B, W), rank-major.  RCCL over xGMI; host-staged only under the test hook."""
        if test_backend:
            buf = torch.empty((world * msg.shape[0], msg.shape[1]), dtype=msg.dtype)
            dist.all_gather_into_tensor(buf, msg.cpu())
            return buf.to(dev)
        buf = torch.empty((world * msg.shape[0], msg.shape[1]), dtype=msg.dtype, device=dev)
        dist.all_gather_into_tensor(buf, msg)
        return buf

    cfg_key, N, width = WORKLOADS[args.workload]
    if args.workload.startswith("synthetic") and not args.items:
        N *= world          # the table lists ONE 8-way shard; the corpus of a run is one such shard per rank
    if args.items:
        N = args.items
    cfg = O.CONFIGS[cfg_key]
    B, k, kp = args.batch, args.k, args.k_prime
    two_pass = args.two_pass > 0
    weights = O.synthetic_weights(cfg, seed=0)
    mol, _ = rails_amd.create_mol_interaction_module(
        cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
        cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
        cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
        query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None)
    mol.load_state_dict(weights, strict=True)
    mol = mol.to(dev).eval()

    lo, hi = shard_bounds(N, world, rank)
    if args.device_table or hi - lo > 4_000_000:
        # the same counter hash, drawn in place in HBM (rails_hash_item_table: bit-equal to the host generator, so any row of any
        # rank's shard is reproducible on a CPU by id)
        X = E.hash_item_table(1, lo, hi - lo, cfg.item_embedding_dim, dev).unsqueeze(0)
        table_kind = "device counter hash (bit-equal to the host generator)"
    else:
        X = torch.from_numpy(O.hash_item_table(1, lo, hi - lo, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
        table_kind = "host counter hash"
    ids = torch.arange(lo + 1, hi + 1, dtype=torch.int64, device=dev).unsqueeze(0)  # 1-based item ids
    q_cpu = O.synthetic_queries(cfg, B)
    q = q_cpu.to(dev)
    uid_cpu = None
    kw = {}
    if len(cfg.uid_embedding_hash_sizes) > 0:
        g = torch.Generator().manual_seed(3)
        uid_cpu = torch.randint(0, cfg.uid_embedding_hash_sizes[0], (B,), generator=g, dtype=torch.int64)
        kw["user_ids"] = uid_cpu.to(dev)

    last_outputs = {}   # leg -> (top_k_ids, top_k_scores) of its last timed step, copied to the host after the timed region (--dump-outputs)
    recall_info = None
    if two_pass and args.full and not args.no_recall:
        # north_star: config 5 "with recall@k vs exact reported".  Untimed, BEFORE the timed module exists (one index per rank at a
        # time: a full shard's is 160 GB): the same two-pass module on planted-structure weights against exact brute force over the
        # whole (sharded) corpus -- every item scored by the fp32 kernels, exact local top-k, the same all-gather + merge.
        with torch.inference_mode():
            mol.load_state_dict({kk: vv.to(dev) for kk, vv in planted_weights(weights).items()}, strict=True)
            mod_p = ShardedMoLAvgTopK(mol, X, ids, N, avg_top_k=args.two_pass)
            k_r = min(k, args.two_pass)
            _, got = mod_p(q, k=k_r, **kw)
            local_p = mod_p._local_module
            hits10 = hitsk = 0
            for b0 in range(0, B, 8):
                lg = local_p.all_logits(q[b0 : b0 + 8], **{kk: vv[b0 : b0 + 8] for kk, vv in kw.items()})
                s_, top_ = E.topk(lg, min(k_r, hi - lo), ids=local_p._ids_flat)
                del lg
                if sharded:
                    s_, top_ = E.merge_candidates(all_gather_rows(E.pack_candidates(s_, top_, k_r)), world, k_r, k_r)
                for r in range(top_.shape[0]):
                    mine, ref = got[b0 + r].tolist(), top_[r].tolist()
                    hits10 += len(set(mine[:10]) & set(ref[:10]))
                    hitsk += len(set(mine) & set(ref))
            recall_info = {"recall@10": hits10 / (B * 10), f"recall@{k_r}": hitsk / (B * k_r), "k": k_r, "queries": B, "avg_top_k_per_shard": args.two_pass,
                           "against": "exact brute-force MoL top-k over the whole corpus (every item of every shard scored by the fp32 kernels, same all-gather + merge)",
                           "weights": "planted structure (gate output layers x 0.25); the timed region below uses the plain random init, where pass 1 is uncorrelated with MoL"}
            del mod_p, local_p
            gc.collect()              # the collector is off (see above): the module's reference cycles would keep its 160 GB index alive
            torch.cuda.empty_cache()
            mol.load_state_dict({kk: vv.to(dev) for kk, vv in weights.items()}, strict=True)

    # Every leg below that drives the fp32 kernels by hand (events around the scoring launch, phase timings, the in-run checks of the sharded
    # path) works on the DENSE binding of the module; the proved mode -- the module's default -- is timed through the module API in its own leg
    # and becomes `value` when it qualifies (see --precision).
    rails_amd.MoLBruteForceTopK.EXACT_MODE = "dense"
    with torch.inference_mode():
        t0 = time.perf_counter()
        if two_pass:
            topk_mod = ShardedMoLAvgTopK(mol, X, ids, N, avg_top_k=args.two_pass)
        else:
            topk_mod = ShardedMoLBruteForceTopK(mol, X, ids, N)
        torch.cuda.synchronize()
        index_build_s = time.perf_counter() - t0
        local = topk_mod._local_module
        eng = local._bind()
        # seen ids: half of each row's own top-k' (so the filter has work) + zero padding
        _, top_ids = topk_mod(q, k=min(kp, N), **kw)
        inv = torch.zeros((B, width), dtype=torch.int64, device=dev)
        g = torch.Generator().manual_seed(4)
        for b in range(B):
            sel = torch.randperm(top_ids.shape[1], generator=g)[: width // 2].to(dev)
            inv[b, : width // 2] = top_ids[b, sel]
        cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)

        ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
        ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
        ev_step = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]   # step boundaries, for the spread
        logits = None if two_pass else torch.empty((B, hi - lo), dtype=torch.float32, device=dev)

        def two_pass_step(i=None):
            """get_top_k_outputs through the (sharded) two-pass module: coarse top-K' + rerank + merge + filter."""
            out_ids, out_scores, _ = cand.get_top_k_outputs(q, k, kw, topk_mod, inv, truncate_k_prime_to=kp)
            return out_ids, out_scores

        def step(i=None):
            """get_top_k_outputs with the scoring launch bracketed by events on the launch stream."""
            qpack, _, _ = eng.query_pack(q, kw.get("user_ids"))
            if i is not None:
                ev0[i].record()
            k_local = min(kp, hi - lo)
            mark = (lambda: ev1[i].record()) if i is not None else (lambda: None)
            eng.score_dense(qpack, B, local._index, out=logits)
            mark()
            if not sharded and E.topk_filter_fusable(hi - lo, k_local, inv.shape[1], k):   # filter fused into the selection over the dense logits
                return E.topk_filtered(logits, k_local, local._ids_flat, inv, k)
            s, top = E.topk(logits, k_local, ids=local._ids_flat)
            if sharded:
                gathered = all_gather_rows(E.pack_candidates(s, top, kp))
                if E.merge_filter_fusable(kp, inv.shape[1], k):   # what the sharded module does: the filter inside the merge launch
                    return E.merge_candidates_filtered(gathered, world, kp, kp, inv, k)
                s, top = E.merge_candidates(gathered, world, kp, kp)
            return E.filter_seen_ids(top, s, inv, k)

        if two_pass:
            step = two_pass_step   # noqa: F811
        else:
            # sanity: the decomposed step equals the module API
            ref_ids, ref_scores, _ = cand.get_top_k_outputs(q, k, kw, topk_mod, inv, truncate_k_prime_to=kp)
            got_ids, got_scores = step()
            assert torch.equal(ref_ids, got_ids) and torch.equal(ref_scores, got_scores)

        def run_pipelined(n):
            """n steps with the exchange of batch i (all-gather, merge) and its filter behind batch i+1's prologue + scoring."""
            # the exact path keeps one batch submitted ahead (its exchange is what overlaps); the two-pass path two: the short launches at
            # the head of a batch then have a whole table scan of the batch before to hide under (MoLAvgTopK.submit)
            depth = 2 if two_pass else 1
            hs = [topk_mod.submit(q, k=min(kp, N), **kw) for _ in range(min(depth, n))]
            submitted = len(hs)
            out = None
            for i in range(n):
                ev_step[i].record()
                if submitted < n:
                    hs.append(topk_mod.submit(q, k=min(kp, N), **kw))
                    submitted += 1
                h = hs.pop(0)
                if E.merge_filter_fusable(min(kp, N), inv.shape[1], k):
                    out = topk_mod.result(h, seen=(inv, k))
                else:
                    s_, top_ = topk_mod.result(h)
                    out = E.filter_seen_ids(top_, s_, inv, k)
            return out

        pipelined_headline = args.pipeline and (sharded or two_pass)
        gc.collect()
        for _ in range(args.warmup):
            step()
        if sharded:
            import torch.distributed as dist

            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if pipelined_headline:
            last_out = run_pipelined(args.steps)
        else:
            for i in range(args.steps):
                ev_step[i].record()
                last_out = step(i)
        ev_step[args.steps].record()
        torch.cuda.synchronize()
        if sharded:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        last_outputs["headline"] = host_copy(last_out)

        sharded_info = None
        if sharded and not two_pass and args.full:
            # what carried the exchange, where a step's time goes (events on the launch stream, unpipelined), and the pipelined rate
            pe = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(args.steps)]
            for i in range(args.steps):
                qpack, _, _ = eng.query_pack(q, kw.get("user_ids"))
                pe[i][0].record()
                eng.score_dense(qpack, B, local._index, out=logits)
                pe[i][1].record()
                s_, top_ = E.topk(logits, min(kp, hi - lo), ids=local._ids_flat)
                msg_ = E.pack_candidates(s_, top_, kp)
                pe[i][2].record()
                gathered_ = all_gather_rows(msg_)
                pe[i][3].record()
                s_, top_ = E.merge_candidates(gathered_, world, kp, kp)
                E.filter_seen_ids(top_, s_, inv, k)
                pe[i][4].record()
            torch.cuda.synchronize()
            phase = [sum(pe[i][j].elapsed_time(pe[i][j + 1]) for i in range(args.steps)) / args.steps for j in range(4)]
            ref_out = step()
            p_out = run_pipelined(2)
            equal = bool(torch.equal(ref_out[0], p_out[0]) and torch.equal(ref_out[1], p_out[1]))
            dist.barrier()
            torch.cuda.synchronize()
            tp = time.perf_counter()
            run_pipelined(args.steps)
            torch.cuda.synchronize()
            dist.barrier()
            p_elapsed = time.perf_counter() - tp
            tpp = torch.tensor([p_elapsed], dtype=torch.float64, device="cpu" if test_backend else dev)
            dist.all_reduce(tpp, op=dist.ReduceOp.MAX)
            # ---- in-run correctness evidence (pytest does not run on the multi-GPU node: the line must carry its own) ----
            k_loc = min(kp, hi - lo)
            qpack, _, _ = eng.query_pack(q, kw.get("user_ids"))
            eng.score_dense(qpack, B, local._index, out=logits)
            ls_, li_ = E.topk(logits, k_loc, ids=local._ids_flat)
            ms_, mi_ = E.merge_candidates(all_gather_rows(E.pack_candidates(ls_, li_, kp)), world, kp, kp)    # merged top-k', before the filter
            fin_i, fin_s = step()

            def gather_i64(t):   # (n,) int64 per rank -> (world, n)
                return all_gather_rows(t.reshape(1, -1).to(torch.int64).contiguous())

            # (1) every rank holds the same final (ids, score bits): a 64-bit mix of both, all-gathered
            mix = (fin_i * 0x9E3779B97F4A7C15 + fin_s.contiguous().view(torch.int32).to(torch.int64) * 0xC2B2AE3D27D4EB4F
                   + torch.arange(fin_i.numel(), device=dev, dtype=torch.int64).view_as(fin_i) * 0x165667B19E3779F9)
            digest = gather_i64(mix.sum().reshape(1))
            all_identical = bool((digest == digest[0]).all())
            # ALL collectives of the check first (every rank runs them unconditionally); the local recompute, which can only fail
            # locally, afterwards -- an exception there must not leave the ranks at different collectives
            rows = X[0].index_select(0, (li_.reshape(-1) - (lo + 1)).clamp(min=0))
            g_rows = all_gather_rows(rows.reshape(1, -1)).view(-1, X.shape[2])
            g_ids = gather_i64(li_.reshape(-1)).reshape(-1)
            # (3) per shard: nothing outside the merged list beats its k'-th score
            kth = ms_[:, -1:]
            above_local = (logits > kth).sum(1)
            mine_in_merged = ((mi_ > lo) & (mi_ <= hi) & (ms_ > kth)).sum(1)
            ok_local = torch.tensor([int(bool((above_local == mine_in_merged).all()))], dtype=torch.int64, device=dev)
            nothing_outside = bool((gather_i64(ok_local) == 1).all())
            # (2) merged == unsharded: ONE device scores the union of every rank's local top-k' rows (a superset of every query's
            #     candidates: anything that beats a query's k'-th overall is in its shard's local top-k') as a corpus of its own and
            #     selects.  Ids sorted ascending = global position order, so ties break as in the whole corpus; the scoring kernels
            #     return the same bits whatever the corpus size (small-unit and 32x32x2 shells alike).
            merged_equals_unsharded, union_items, check_error = None, None, None
            try:
                u_ids = torch.unique(g_ids, sorted=True)
                order = torch.argsort(g_ids, stable=True)
                keep = torch.ones_like(order, dtype=torch.bool)
                keep[1:] = g_ids[order][1:] != g_ids[order][:-1]
                u_rows = g_rows[order][keep]
                assert u_rows.shape[0] == u_ids.numel()
                union = rails_amd.MoLBruteForceTopK(mol, u_rows.unsqueeze(0).contiguous(), u_ids.unsqueeze(0))
                us_, ui_ = union(q, k=kp, **kw)
                merged_equals_unsharded = bool(torch.equal(us_, ms_) and torch.equal(ui_, mi_))
                union_items = int(u_ids.numel())
                del union
            except Exception as e:   # noqa: BLE001 -- a failure OF the check (not a failed check) is reported, it does not void the timing
                check_error = f"{type(e).__name__}: {e}"[:300]
            sharded_check = {"all_ranks_identical": all_identical, "merged_equals_unsharded": merged_equals_unsharded,
                             "nothing_outside_beats_kth": nothing_outside, "union_items": union_items,
                             "how": "digest of (ids, score bits) all-gathered; union of every rank's local top-k' rows re-scored and re-selected on one device; "
                                    "per-shard count of logits above the merged k'-th"}
            if check_error:
                sharded_check["error"] = check_error
            if not all_identical or merged_equals_unsharded is False or not nothing_outside:
                raise SystemExit(f"sharded result failed its in-run check: {sharded_check}")
            sharded_info = {
                "check": sharded_check,
                "backend": dist.get_backend(), "rccl_ranks": dist.get_world_size(),
                "exchange": "one all_gather_into_tensor of (B, 2k') int64 per batch" + (" (host-staged: test hook)" if test_backend else " on device tensors"),
                "message_bytes_per_rank": B * 2 * kp * 8,
                "phase_ms": {"score": phase[0], "select_and_pack": phase[1], "all_gather": phase[2], "merge_and_filter": phase[3]},
                "pipelined": {"ms_per_step": float(tpp.item()) / args.steps * 1e3, "value": B * args.steps / float(tpp.item()), "unit": "queries/s",
                              "output_equal_to_unpipelined": equal, "headline_uses_it": bool(pipelined_headline)},
            }
        if sharded and two_pass and args.full:
            # the approximate mode has no unsharded twin to equal (K' per shard); what the line can carry is that every rank ends with
            # the same (ids, score bits), plus the recall measurement above
            fin_i, fin_s = step()
            mix = (fin_i * 0x9E3779B97F4A7C15 + fin_s.contiguous().view(torch.int32).to(torch.int64) * 0xC2B2AE3D27D4EB4F
                   + torch.arange(fin_i.numel(), device=dev, dtype=torch.int64).view_as(fin_i) * 0x165667B19E3779F9)
            digest = all_gather_rows(mix.sum().reshape(1, 1))
            same = bool((digest == digest[0]).all())
            if not same:
                raise SystemExit("sharded two-pass result differs between ranks")
            sharded_info = {"check": {"all_ranks_identical": same}, "backend": dist.get_backend(), "rccl_ranks": dist.get_world_size(),
                            "exchange": "one all_gather_into_tensor of (B, 2k') int64 per batch" + (" (host-staged: test hook)" if test_backend else " on device tensors")}
        per_step_ms = [ev_step[i].elapsed_time(ev_step[i + 1]) for i in range(args.steps)]
        two_pass_pipelined = None
        if two_pass and args.full:
            # MoLAvgTopK.submit / result: batch i + 1 is enqueued before the host looks at batch i's verdict word (the fused scan's
            # candidate counts), so that look costs the GPU nothing; same launches, same output
            ref_out = step()
            p_out = run_pipelined(max(2, args.warmup))
            equal = bool(torch.equal(ref_out[0], p_out[0]) and torch.equal(ref_out[1], p_out[1]))
            if sharded:
                dist.barrier()
            torch.cuda.synchronize()
            tp = time.perf_counter()
            run_pipelined(args.steps)
            torch.cuda.synchronize()
            if sharded:
                dist.barrier()
            p_elapsed = time.perf_counter() - tp
            if sharded:
                tpp = torch.tensor([p_elapsed], dtype=torch.float64, device="cpu" if test_backend else dev)
                dist.all_reduce(tpp, op=dist.ReduceOp.MAX)
                p_elapsed = float(tpp.item())
            two_pass_pipelined = {"ms_per_step": p_elapsed / args.steps * 1e3, "value": B * args.steps / p_elapsed, "unit": "queries/s",
                                  "output_equal_to_unpipelined": equal, "headline_uses_it": bool(pipelined_headline),
                                  "what": "two batches submitted ahead of the one whose result is taken: the host reads a batch's verdict word while the GPU runs the next ones, whose short launches run under its table scan"}
        score_ms = None       # two-pass: the coarse scan's own timing below is a --full measurement
        if two_pass and args.full:
            # the dominant kernel chain of this mode is the fused coarse top-K' (HBM-bound scan of the bf16 table):
            # timed on its own, on the launch stream, after the step timing
            table = local._table()
            _, eq_plain, _ = eng.query_pack(q, kw.get("user_ids"), want_plain=True)
            kp_local = min(args.two_pass, hi - lo)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pre = local._prefilter(count=False)          # the int8 copy the streaming pass reads instead of the bf16 table (large tables)
            eng.coarse_topk(eq_plain, table, False, kp_local, prefilter=pre)
            e0.record()
            for _ in range(args.steps):
                eng.coarse_topk(eq_plain, table, False, kp_local, prefilter=pre)
            e1.record()
            torch.cuda.synchronize()
            score_ms = e0.elapsed_time(e1) / args.steps
            bf16_table_bytes = table.numel() * table.element_size()
            # algorithmic bytes of the pass = what its streaming launch has to read once: the int8 copy (d bytes per item) when
            # there is one, else the bf16 table (2d)
            coarse_table_bytes = (pre.numel() - 256) if pre is not None else bf16_table_bytes
            score_ms_bf16 = None
            if pre is not None:
                e0.record()
                for _ in range(args.steps):
                    eng.coarse_topk(eq_plain, table, False, kp_local)
                e1.record()
                torch.cuda.synchronize()
                score_ms_bf16 = e0.elapsed_time(e1) / args.steps
        elif not two_pass:
            score_ms = sum(a.elapsed_time(b) for a, b in zip(ev0, ev1)) / args.steps

        nofilter_elapsed = None
        if args.full:
            # the same step without the seen-id filter (k' = k, invalid_ids = None), timed the same way
            # after the headline region
            def step_nofilter():
                out_ids, out_scores, _ = cand.get_top_k_outputs(q, k, kw, topk_mod, None)
                return out_ids

            for _ in range(args.warmup):
                step_nofilter()
            if sharded:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step_nofilter()
            torch.cuda.synchronize()
            if sharded:
                dist.barrier()
            nofilter_elapsed = time.perf_counter() - t0
            if sharded:
                tn = torch.tensor([nofilter_elapsed], dtype=torch.float64, device="cpu" if test_backend else dev)
                dist.all_reduce(tn, op=dist.ReduceOp.MAX)
                nofilter_elapsed = float(tn.item())

        # ---- the PROVED exact path (the module's default): same step through the module API, same protocol (W warm-up steps, K timed steps
        #      between barrier + synchronize), the first-pass launch bracketed by events on its stream.  Its output must equal the dense
        #      fp32 step's bit for bit and every timed call must have been proved on the device for it to become `value`.
        proved = None
        if not two_pass and args.precision == "proved":
            local.exact_mode = "proved"
            eng_p = local._bind()
            mod_stats = topk_mod.stats if hasattr(topk_mod, "stats") else local.stats     # N > 1: the sharded module's global proof keeps the counters
            if eng_p.exact is not None:
                pe0 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
                pe1 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
                p_step = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
                cur = {"i": None}
                local._first_pass_hook = lambda w: (pe0 if w == 0 else pe1)[cur["i"]].record() if cur["i"] is not None else None

                def step_proved(i=None):
                    cur["i"] = i
                    out_ids, out_scores, _ = cand.get_top_k_outputs(q, k, kw, topk_mod, inv, truncate_k_prime_to=kp)
                    return out_ids, out_scores

                p_ids, p_scores = step_proved()
                p_identical = bool(torch.equal(p_ids, ref_ids) and torch.equal(p_scores, ref_scores))
                gc.collect()
                # settle first: a failed verdict doubles the candidate margin for the calls after it, and a shard's k'-th score sits in a denser
                # part of the score distribution than the whole corpus' -- calls until two in a row were proved (at most 12; every rank runs the
                # same count: the fallback counter is max-reduced).  These calls read counters back (host syncs).
                for _ in range(2):
                    step_proved()
                for _ in range(6):
                    before = mod_stats()["fallbacks"]
                    step_proved()
                    step_proved()
                    failed = torch.tensor([mod_stats()["fallbacks"] - before], dtype=torch.int64, device="cpu" if (sharded and test_backend) else dev)
                    if sharded:
                        dist.all_reduce(failed, op=dist.ReduceOp.MAX)
                    if int(failed.item()) == 0:
                        break
                mod_stats()
                base_stats = dict(mod_stats())
                # ... then the W warm-up steps, with nothing but the barrier + synchronize between them and the timed region: the f16 kernel
                # loses its clocks within milliseconds of idle and takes ~8 steps to get them back (tools/r05_ramp_probe.py), so counters
                # are read BEFORE the warm-up (the W calls are subtracted below) and not between warm-up and timing
                n_warm = max(args.warmup, 0)
                for _ in range(n_warm):
                    step_proved()
                if sharded:
                    dist.barrier()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    p_step[i].record()
                    p_last = step_proved(i)
                p_step[args.steps].record()
                torch.cuda.synchronize()
                if sharded:
                    dist.barrier()
                p_elapsed = time.perf_counter() - t0
                last_outputs["proved"] = host_copy(p_last)
                if sharded:
                    tpv = torch.tensor([p_elapsed], dtype=torch.float64, device="cpu" if test_backend else dev)
                    dist.all_reduce(tpv, op=dist.ReduceOp.MAX)
                    p_elapsed = float(tpv.item())
                local._first_pass_hook = None
                cur["i"] = None
                st = mod_stats()
                p_last_ids, p_last_scores = step_proved()
                p_identical = p_identical and bool(torch.equal(p_last_ids, ref_ids) and torch.equal(p_last_scores, ref_scores))
                # N > 1: the same K steps with batch i + 1 submitted before batch i's result is taken (ShardedTopK.submit / result): the plain call
                # waits on the host for the global verdict behind its one all-gather; with a batch in flight that wait costs the GPU nothing
                p_pipe = None
                if sharded and not two_pass and hasattr(topk_mod, "submit") and (args.full or args.pipeline):
                    pp_out = run_pipelined(2)
                    pp_equal = bool(torch.equal(pp_out[0], ref_ids) and torch.equal(pp_out[1], ref_scores))
                    pp_before = dict(mod_stats())
                    dist.barrier()
                    torch.cuda.synchronize()
                    tpp0 = time.perf_counter()
                    pp_last = run_pipelined(args.steps)
                    torch.cuda.synchronize()
                    dist.barrier()
                    pp_elapsed = time.perf_counter() - tpp0
                    last_outputs["proved_pipelined"] = host_copy(pp_last)
                    tpp_t = torch.tensor([pp_elapsed], dtype=torch.float64, device="cpu" if test_backend else dev)
                    dist.all_reduce(tpp_t, op=dist.ReduceOp.MAX)
                    pp_elapsed = float(tpp_t.item())
                    pp_after = mod_stats()
                    pp_counts = torch.tensor([pp_after["calls"] - pp_before["calls"], pp_after.get("proved_calls", 0) - pp_before.get("proved_calls", 0),
                                              pp_after["fallbacks"] - pp_before["fallbacks"], int(pp_equal)], dtype=torch.int64, device="cpu" if test_backend else dev)
                    dist.all_reduce(pp_counts, op=dist.ReduceOp.SUM)
                    pc, pv, pf, pe_ = (int(v) for v in pp_counts.tolist())
                    p_pipe = {"ms_per_step": pp_elapsed / args.steps * 1e3, "queries_per_s": B * args.steps / pp_elapsed, "timed_calls": pc, "proved_calls": pv,
                              "dense_fp32_fallbacks": pf, "output_equal_to_unpipelined": pe_ == world,
                              "what": "the same K proved steps with batch i + 1 submitted before batch i's result is taken (depth 1): every result verified before it is returned"}
                # warm-up + timed calls since the snapshot; the timed ones are "all proved" only if every call since the snapshot was
                since_calls = st["calls"] - base_stats["calls"]
                since_proved = st.get("proved_calls", 0) - base_stats.get("proved_calls", 0)
                timed_calls = since_calls - n_warm
                timed_proved = args.steps if (since_proved == since_calls and timed_calls == args.steps) else max(0, min(since_proved - n_warm, timed_calls - (st["fallbacks"] - base_stats["fallbacks"])))
                counts = torch.tensor([timed_calls, timed_proved, st["fallbacks"] - base_stats["fallbacks"],
                                       st.get("bound_violations", 0), int(p_identical)], dtype=torch.int64, device="cpu" if (sharded and test_backend) else dev)
                if sharded:          # every rank's shard must have been proved
                    dist.all_reduce(counts, op=dist.ReduceOp.SUM)
                timed_calls, proved_calls, fallbacks, violations, identical_ranks = (int(v) for v in counts.tolist())
                p_score_ms = sum(a.elapsed_time(b) for a, b in zip(pe0, pe1)) / args.steps
                p_steps_ms = [p_step[i].elapsed_time(p_step[i + 1]) for i in range(args.steps)]
                p_kernel_ms = [a.elapsed_time(b) for a, b in zip(pe0, pe1)]
                proved = {"elapsed": p_elapsed, "score_ms": p_score_ms, "steps_ms": p_steps_ms, "kernel_ms": p_kernel_ms, "calls": timed_calls, "proved_calls": proved_calls, "fallbacks": fallbacks,
                          "bound_violations": violations, "identical": identical_ranks == world, "eps": st.get("eps_rigorous"), "eps_terms": st.get("eps_rigorous_terms"),
                          "bound_kind": st.get("bound_kind", "one a-priori eps"), "upper_bound_poly": st.get("upper_bound_poly"),
                          "kc": st.get("kc"), "guard_max": st.get("guard_max"), "guard_limit": getattr(topk_mod, "_gp_guard_limit", None) if st.get("global_proof") else local._gate_guard_limit,
                          "global_proof": bool(st.get("global_proof", False)), "pipelined": p_pipe,
                          "qualifies": bool(identical_ranks == world and proved_calls == timed_calls == args.steps * world and fallbacks == 0 and violations == 0)}
            local.exact_mode = "dense"
            eng = local._bind()       # the legs below drive the fp32 kernels by hand again

    # ---- opt-in precision mode "f16x3" (same API, same index, same 1e-4 bar), timed the same
    #      way AFTER the headline region so it cannot perturb it.  Reported separately; `value` stays the exact-fp32 path.
    fast = None
    if args.full and not args.no_fast_path and not two_pass:
        with torch.inference_mode():
            # the exact-fp32 logits to compare with (the fused headline step does not write them)
            eng.score_dense(eng.query_pack(q, kw.get("user_ids"))[0], B, local._index, out=logits)
            mol.precision = "f16x3"
            eng = local._bind()          # new engine (split weight fragments); the item index is rebuilt in the same format
            d_logits = torch.empty_like(logits)
            qp, _, _ = eng.query_pack(q, kw.get("user_ids"))
            eng.score_dense(qp, B, local._index, out=d_logits)
            max_dev = float((d_logits - logits).abs().max())   # vs the exact-fp32 logits of the last headline step
            # do the two precisions return the same items?  top-k' of both logit matrices over this rank's whole shard
            k_cmp = min(kp, hi - lo)
            _, ids32 = E.topk(logits, k_cmp, ids=local._ids_flat)
            _, ids16 = E.topk(d_logits, k_cmp, ids=local._ids_flat)
            same_rank = float((ids32 == ids16).float().mean())
            same_set = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ids32.cpu(), ids16.cpu())) / ids32.numel()
            ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
            ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
            for _ in range(args.warmup):
                step()
            if sharded:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(i)
            torch.cuda.synchronize()
            if sharded:
                dist.barrier()
            fast_elapsed = time.perf_counter() - t0
            fast_ms = sum(a.elapsed_time(b) for a, b in zip(ev0, ev1)) / args.steps
            mol.precision = None
        if sharded:
            tf = torch.tensor([fast_elapsed], dtype=torch.float64, device="cpu" if test_backend else dev)
            dist.all_reduce(tf, op=dist.ReduceOp.MAX)
            fast_elapsed = float(tf.item())
        fast = {
            "precision": "f16x3: gate GEMMs + sub-embedding contraction on f16 MFMA, operands split hi+lo, 3 MFMAs per block, fp32 accumulate",
            "value": B * args.steps / fast_elapsed, "unit": "queries/s", "ms_per_step": fast_elapsed / args.steps * 1e3,
            "kernel_ms": fast_ms, "achieved_tflops_algorithmic": B * (hi - lo) * flops_per_pair(cfg) / (fast_ms * 1e-3) / 1e12,
            "max_abs_logit_diff_vs_fp32_path": max_dev,
            f"top{k_cmp}_ids_identical_to_fp32_path": {"same_item_at_same_rank": same_rank, "same_item_set": same_set,
                                                         "note": "differences are swaps inside groups of fp32 logits closer than the two paths' rounding (~2e-5)"},
        }
        a16 = fast["achieved_tflops_algorithmic"]
        fast["roofline"] = {"kernel": "mol_score_*_kernel<F16Unit>", "bound": "mfma", "achieved": a16, "peak": PEAK_F16X3_TFLOPS, "unit": "TFLOP/s",
                            "frac": a16 / PEAK_F16X3_TFLOPS,
                            "traffic": committed_traffic(f"{args.workload}:B{B}:gpus{world}:f16x3"),
                            "traffic_source": "profiles/pmc_summary.json (rocprofv3 --pmc passes of this kernel and workload; not collected in this run)",
                            "hbm_bytes_alg_per_launch": (hi - lo) * bytes_per_item_fp32(cfg) + B * (hi - lo) * 4,
                            "peak_note": "2500 TFLOP/s dense f16 MFMA / 3 MFMAs per product block; issued-MFMA rate = 3 x achieved"}

    # ---- precisions "f16x3-exact" / "f16-exact": the f16x3 (or one-product f16) kernels pick k' + margin candidates per query, the
    #      fp32 kernels re-score them, the result is verified to be the fp32 path's (rails_amd/topk_modules.py _forward_rescored).
    #      Through the module API, compared bit for bit with the headline path's output, timed the same way.  Reported separately.
    exact_fast = None
    if args.full and not args.no_fast_path and not two_pass:
        exact_fast = {}
        for mode, what in (("f16-exact", "one-product f16 scoring of the whole index (logits ~1e-2 off)"), ("f16x3-exact", "f16x3 scoring of the whole index")):
            with torch.inference_mode():
                mol.precision = mode
                local.stats()
                local.rescore_stats.update({"calls": 0, "fallbacks": 0, "audited": 0, "mismatches": 0})

                def step_exact():
                    out_ids, out_scores, _ = cand.get_top_k_outputs(q, k, kw, topk_mod, inv, truncate_k_prime_to=kp)
                    return out_ids, out_scores

                gc.collect()
                x_ids, x_scores = step_exact()
                identical = bool(torch.equal(x_ids, ref_ids) and torch.equal(x_scores, ref_scores))
                for _ in range(args.warmup):
                    step_exact()
                if sharded:
                    dist.barrier()
                torch.cuda.synchronize()
                dbg = os.environ.get("RAILS_BENCH_DEBUG")
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)] if dbg else None
                t0 = time.perf_counter()
                for i_ in range(args.steps):
                    if dbg:
                        evs[i_].record()
                    step_exact()
                if dbg:
                    evs[args.steps].record()
                torch.cuda.synchronize()
                if sharded:
                    dist.barrier()
                exact_elapsed = time.perf_counter() - t0
                if dbg:
                    print(mode, "per-step ms:", [round(a.elapsed_time(b), 2) for a, b in zip(evs, evs[1:])], "pad_scale", local._pad_scale, "pause", local._pause_left,
                          "index32", local._index32 is not None, file=sys.stderr)
                stats = dict(local.stats())
                # shadow audit (not timed): the same step with every call also run on the dense fp32 path on a side stream and compared
                local.audit_every = 1
                for _ in range(min(args.steps, 5)):
                    step_exact()
                audit = local.stats()
                local.audit_every = 0
                stats["audited"], stats["mismatches"] = audit["audited"], audit["mismatches"]
                mol.precision = None
            if sharded:
                tf = torch.tensor([exact_elapsed], dtype=torch.float64, device="cpu" if test_backend else dev)
                dist.all_reduce(tf, op=dist.ReduceOp.MAX)
                exact_elapsed = float(tf.item())
            exact_fast[mode] = {
                "precision": f"{mode}: {what} -> top (k' + margin) candidates per query -> fp32 re-scoring of the candidates -> verified "
                             "fp32 top-k' (dense fp32 fallback when the verification fails)",
                "value": B * args.steps / exact_elapsed, "unit": "queries/s", "ms_per_step": exact_elapsed / args.steps * 1e3,
                "output_identical_to_fp32_path": identical, "rescore_calls": stats["calls"], "dense_fp32_fallbacks": stats["fallbacks"],
                "shadow_audit": {"audited_calls": stats["audited"], "mismatches": stats["mismatches"]}, "eps": stats.get("eps"),
                "eps_rigorous": stats.get("eps_rigorous"), "eps_rigorous_usable": stats.get("eps_rigorous_usable"),
                "proved_calls": stats.get("proved_calls"),
                "guarantee": "conditional on the monitored empirical bound eps (the one-product pass has no useful a-priori bound: rails_amd/topk_modules.py rigorous_eps)"
                             if not stats.get("eps_rigorous_usable") else "proved per call: the verdicts run on the a-priori bound eps_rigorous (rails_amd/f16x3_bound.py)",
            }

    if sharded:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if test_backend else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    n_shard = hi - lo
    flops_alg = B * n_shard * flops_per_pair(cfg)
    achieved = None if score_ms is None else flops_alg / (score_ms * 1e-3) / 1e12

    if rank == 0:
        traffic = None
        pmc = os.path.join(ROOT, "profiles", "pmc_summary.json")
        if os.path.exists(pmc):
            try:
                rec = json.load(open(pmc)).get(f"{args.workload}:B{B}:gpus{world}")
                traffic = rec and rec.get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        out = {
            "metric": "queries/sec, MoL exact top-k over N items (get_top_k_outputs: score + top-k' + id map + seen-id filter)",
            "value": B * args.steps / elapsed,
            "unit": "queries/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "ms_per_step_stdev": float(torch.tensor(per_step_ms).std()) if len(per_step_ms) > 1 else 0.0,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"{args.workload} HSTU+MoL {cfg.query_dot_product_groups}x{cfg.item_dot_product_groups}x{cfg.dot_product_dimension}, N={N} items, exact brute-force top-k",
                "global_batch": B, "k": k, "k_prime": kp, "seen_id_width": width, "n_items": N,
                "parallelism": f"item-shard x{world}" if sharded else "single GPU",
            },
            "roofline": None if score_ms is None else {      # (a plain two-pass run: the coarse scan is timed with --full only)
                "kernel": "mol_score_kernel",
                "bound": "mfma",
                "achieved": achieved,
                "peak": PEAK_F32_MFMA_TFLOPS,
                "unit": "TFLOP/s",
                "frac": achieved / PEAK_F32_MFMA_TFLOPS,
                "traffic": traffic,
                "traffic_source": "profiles/pmc_summary.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same kernel and workload, corrected as MI355X_MICROARCH.md prescribes; not collected in this run)" if traffic else None,
                "kernel_ms": score_ms,
                "flops_per_launch": flops_alg,
                "hbm_bytes_alg_per_launch": n_shard * bytes_per_item_fp32(cfg),
                "hbm_frac": n_shard * bytes_per_item_fp32(cfg) / (score_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS,
            },
            "index_build_s": index_build_s,
        }
        out["config"]["item_table"] = table_kind
        value_leg = "headline"    # the leg whose timed steps `value` reports (--dump-outputs writes its last step)
        if not two_pass:
            out["config"]["exact_path"] = "dense fp32 kernels over the whole corpus"
        if proved is not None:
            p_val = B * args.steps / proved["elapsed"]
            a16 = flops_alg / (proved["score_ms"] * 1e-3) / 1e12
            leg = {
                "what": "the module's default exact path: split-f16 (f16x3) first pass over the whole corpus -> threshold selection of at most kc candidates per query "
                        "(one histogram + one compaction launch) -> fp32 re-scoring of the candidates -> one finish launch: top-k' by (fp32 score, position), seen-id filter, "
                        "device-side proof UNDER THE MEASURED ARITHMETIC MODEL (hypotheses H1-H3 of rails_amd/f16x3_bound.py, re-checked on this device when the module binds): " + (
                            "e_k > m, the first pass having written per-pair UPPER BOUNDS of the fp32 logits (its logit + a bound quadratic in the pair's largest "
                            "|cross logit|: rails_mol_score_dense_upper, f16x3_bound.upper_bound_poly)" if proved.get("upper_bound_poly") else
                            "e_k > m + eps with the A-PRIORI bound eps on |first pass - fp32| (rails_amd/f16x3_bound.py)") +
                        "; a call that is not proved is redone by the dense fp32 kernels behind the verdict",
                "value": p_val, "unit": "queries/s", "ms_per_step": proved["elapsed"] / args.steps * 1e3,
                "ms_per_step_stdev": float(torch.tensor(proved["steps_ms"]).std()) if len(proved["steps_ms"]) > 1 else 0.0,
                "timed_calls": proved["calls"], "proved_calls": proved["proved_calls"], "dense_fp32_fallbacks": proved["fallbacks"],
                "bound_violations": proved["bound_violations"], "output_identical_to_fp32_path": proved["identical"],
                "eps_a_priori": proved["eps"], "bound": proved.get("bound_kind"), **({"upper_bound_poly": proved["upper_bound_poly"]} if proved.get("upper_bound_poly") else {}),
                "candidates_per_query": proved["kc"], "gate_guard": {"max_abs_gq_seen": proved["guard_max"], "limit": proved["guard_limit"]},
                "first_pass_kernel_ms": proved["score_ms"], "is_headline": proved["qualifies"],
                **({"sharded_global_proof": "one proof for all shards: kc per rank = candidates_per_query; ONE all-gather of (B, 2k' + 2) messages -- the per-shard fp32 top-k', "
                                            "the best first-pass score left outside and the largest observed error ride in it -- then merge + verdict + filter in one launch "
                                            "(rails_amd/sharded.py ShardedMoLBruteForceTopK)"} if proved.get("global_proof") else {}),
                **({"pipelined": proved["pipelined"]} if proved.get("pipelined") else {}),
                "per_step_ms": [round(v, 3) for v in proved["steps_ms"]],
                "per_step_first_pass_kernel_ms": [round(v, 3) for v in proved["kernel_ms"]],
                # the f16 kernel's time falls for the first ~40 ms of sustained load after an idle gap (clock ramp; the fp32 kernels do not show it):
                # the second half of the timed steps on its own -- `value` stays the whole timed region
                "second_half": {"ms_per_step": sum(proved["steps_ms"][args.steps // 2:]) / max(1, args.steps - args.steps // 2),
                                "first_pass_kernel_ms": sum(proved["kernel_ms"][args.steps // 2:]) / max(1, args.steps - args.steps // 2)},
            }
            if proved["qualifies"]:
                # `value` = the proved path; the returned scores ARE the fp32 kernels' bits (dtype f32); the dense fp32 measurement of this run moves beside it
                out["fp32_dense"] = {"value": out["value"], "unit": "queries/s", "ms_per_step": out["ms_per_step"], "ms_per_step_stdev": out["ms_per_step_stdev"],
                                     "roofline": out["roofline"], "what": "the dense fp32 kernels over the whole corpus (exact_mode 'dense'), same step, same protocol, timed in this run"}
                out["value"], out["ms_per_step"], out["ms_per_step_stdev"] = leg["value"], leg["ms_per_step"], leg["ms_per_step_stdev"]
                value_leg = "proved"
                pp = proved.get("pipelined")
                if args.pipeline and pp and pp["output_equal_to_unpipelined"] and pp["proved_calls"] == pp["timed_calls"] and pp["dense_fp32_fallbacks"] == 0:
                    # --pipeline: the headline is the rate with one batch in flight (the plain rate stays in `proved`)
                    out["value"], out["ms_per_step"] = pp["queries_per_s"], pp["ms_per_step"]
                    value_leg = "proved_pipelined"
                    out["config"]["pipelined"] = "batch i + 1 submitted before batch i's result is taken (ShardedTopK.submit / result)"
                kind = "per-pair a-priori upper bound" if proved.get("upper_bound_poly") else "a-priori eps"
                out["config"]["exact_path"] = (f"proved under the measured arithmetic model (H1-H3 re-checked on this device): f16x3 first pass + fp32 re-scoring, {kind} "
                                               "(same bits as the dense fp32 kernels)")
                out["config"]["prefilter"] = f"f16x3, {kind}"
                out["roofline"] = {
                    "kernel": "mol_score_*_kernel<f16x3::F16Unit> (the first pass: the dominant launch of the proved step)", "bound": "mfma", "achieved": a16,
                    "peak": PEAK_F16X3_TFLOPS, "unit": "TFLOP/s", "frac": a16 / PEAK_F16X3_TFLOPS,
                    "traffic": committed_traffic(f"{args.workload}:B{B}:gpus{world}:f16x3"),
                    "traffic_source": "profiles/pmc_summary.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this kernel and workload; not collected in this run)",
                    "kernel_ms": proved["score_ms"], "flops_per_launch": flops_alg,
                    "hbm_bytes_alg_per_launch": n_shard * bytes_per_item_fp32(cfg) + B * n_shard * 4,
                    "hbm_frac": (n_shard * bytes_per_item_fp32(cfg) + B * n_shard * 4) / (proved["score_ms"] * 1e-3) / 1e9 / PEAK_HBM_GBPS,
                    "peak_note": "2500 TFLOP/s dense f16 MFMA / 3 MFMAs per algorithmic product block; issued-MFMA rate = 3 x achieved",
                }
            out["proved"] = leg
        if nofilter_elapsed is not None:
            out["without_seen_id_filter"] = {"value": B * args.steps / nofilter_elapsed, "unit": "queries/s",
                                             "ms_per_step": nofilter_elapsed / args.steps * 1e3, "k": k}
        if two_pass:
            out["metric"] = "queries/sec, MoL two-pass approximate top-k over N items (get_top_k_outputs: coarse top-K' + MoL rerank + id map + seen-id filter)"
            out["config"]["workload"] = (f"{args.workload} MoL {cfg.query_dot_product_groups}x{cfg.item_dot_product_groups}x{cfg.dot_product_dimension}, "
                                         f"N={N} items, two-pass MoLAvgTopK, K'={args.two_pass} per shard")
            out["config"]["avg_top_k_per_shard"] = args.two_pass
            out["scaling"] = "weak" if args.workload.startswith("synthetic") and not args.items else "strong"
        if two_pass_pipelined is not None:
            out["pipelined"] = two_pass_pipelined
        if two_pass and score_ms is not None:     # --full: the fused coarse top-K' timed on its own
            gbps = coarse_table_bytes / (score_ms * 1e-3) / 1e9
            out["roofline"] = {
                "kernel": ("coarse_scan_i8_kernel (fused coarse top-K': sample pass + select pass over the int8 copy of the table, fired tiles from the bf16 table + key selection)"
                           if score_ms_bf16 is not None else "coarse_scan_kernel (fused coarse top-K': sample pass + select pass + key selection)"),
                "bound": "hbm", "achieved": gbps, "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": gbps / PEAK_HBM_GBPS,
                "traffic": None, "kernel_ms": score_ms, "hbm_bytes_alg_per_launch": coarse_table_bytes,
            }
            if score_ms_bf16 is not None:
                out["roofline"]["without_int8_prefilter"] = {"kernel_ms": score_ms_bf16, "hbm_bytes_alg_per_launch": bf16_table_bytes,
                                                             "achieved": bf16_table_bytes / (score_ms_bf16 * 1e-3) / 1e9, "frac": bf16_table_bytes / (score_ms_bf16 * 1e-3) / 1e9 / PEAK_HBM_GBPS}
            if args.workload == "synthetic-8x8x32" and hi - lo == 125_000_000 and B in (32, 128):
                # committed PMC passes of the select scan (the launch that reads the table; the time above also covers the sample
                # pass and the key selection)
                tr = (committed_traffic(f"synthetic-8x8x32:coarse_scan_i8:N125M:B{B}:r04") if score_ms_bf16 is not None else None) or \
                    (None if score_ms_bf16 is not None else (committed_traffic(f"synthetic-8x8x32:coarse_scan:N125M:B{B}:r04") or committed_traffic(f"synthetic-8x8x32:coarse_scan:N125M:B{B}:r03")))
                if tr:
                    out["roofline"]["traffic"] = tr
                    out["roofline"]["traffic_source"] = ("profiles/pmc_summary.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the select-scan launch on this "
                                                         "workload; FETCH_SIZE x 2 on gfx950; not collected in this run)")
        if two_pass and recall_info is not None:
            out["recall"] = recall_info
        if sharded_info is not None:
            out["sharded"] = sharded_info
        if fast is not None:
            out["fast_path"] = fast
        if exact_fast is not None:
            out["exact_fast_path"] = exact_fast
        if args.full and not sharded and not two_pass and not args.no_matrix:
            # the other points of the reference's protocol on this workload -- small batches (B = 1 is the
            # HBM-bound end: one index pass per query) and the accuracy protocol (k = 2500 -> k' = 2561, no truncation)
            out["matrix"] = measurement_matrix(mol, X, ids, q, kw, inv, cfg, hi - lo, min(args.steps, 10), dev)
        if args.full and not sharded and args.workload == "amzn-books" and not args.no_other_workloads:
            # the two smaller real-dataset shapes of BASELINE.json (configs 1 and 2): fixed per-batch costs dominate there
            out["other_workloads"] = [quick_workload(n, B, k, kp, 10, dev, precision=pr) for n in ("ml-20m", "ml-1m") for pr in ("fp32", "proved", "f16x3", "f16-exact")]
            # BASELINE config 4 (16x16x64, 100 M items 8-way): a 400 k-item sub-range of one shard -- the kernels are linear in N
            out["other_workloads"] += [quick_workload("synthetic-16x16x64", B, k, kp, 5, dev, items=400_000, precision=pr) for pr in ("fp32", "proved", "f16x3", "f16-exact")]
        if args.full and not sharded and not two_pass and not args.no_weights_sweep and args.precision == "proved":
            try:
                out["weights_scale_sweep"] = weights_scale_sweep(cfg, weights, X, ids, q, kw, inv, k, kp, min(args.steps, 10), dev)
            except Exception as e:   # noqa: BLE001 -- a secondary leg must not take the headline line down with it
                out["weights_scale_sweep"] = [{"skipped": f"{type(e).__name__}: {e}"[:300]}]
                torch.cuda.empty_cache()
        if args.full and not sharded and args.workload == "amzn-books" and not args.no_other_workloads and not args.no_full_shards:
            try:
                out["full_shards"] = full_shard_legs(B, k, dev)
            except Exception as e:   # noqa: BLE001 -- a secondary leg must not take the headline line down with it (e.g. a smaller device)
                out["full_shards"] = [{"skipped": f"{type(e).__name__}: {e}"[:300]}]
                torch.cuda.empty_cache()
        shared = None
        if args.full and not sharded and not args.no_cpu_baseline and not two_pass:   # the CPU baseline is the exact path
            cb = cpu_baseline(cfg, weights, q_cpu, uid_cpu, N, min(args.cpu_sample_items or N, N), kp)
            oracle_topk = cb.pop("_oracle_topk")
            out["cpu_baseline"] = cb
            if oracle_topk is not None and kp == 200 and k == 120:
                shared = (q_cpu, uid_cpu, N, oracle_topk)
        if args.full and not sharded and not two_pass and not args.no_hr_parity:
            # the quality half of the metric + the reference's own CSV line (eval_from_checkpoint.py:507-515; BatchTimeMs = this run's step)
            hp = hr_parity_leg(cfg, weights, mol, B, 120, 200, dev, shared=shared,    # the harness's own timing-protocol constants (data/eval.py:128-130)
                               exact_mode="proved" if (proved is not None and proved["qualifies"]) else "dense")
            out["hr_parity"] = hp
            out["reference_csv"] = {"header": "HR@1,HR@5,HR@10,HR@50,HR@100,BatchTimeMsAvg,BatchTimeMsDev",
                                    "row": ",".join([f"{hp[m]['hip']}" for m in ("hr@1", "hr@5", "hr@10", "hr@50", "hr@100")]
                                                    + [f"{out['ms_per_step']:.3f}", f"{out['ms_per_step_stdev']:.3f}"]),
                                    "oracle_row": ",".join(f"{hp[m]['oracle']}" for m in ("hr@1", "hr@5", "hr@10", "hr@50", "hr@100")),
                                    "note": "HR columns: hr_parity corpus with planted targets (HIP path; oracle_row = the CPU oracle chain on the same inputs); "
                                            "time columns: the headline step of this run"}
        if args.dump_outputs:
            top_ids, top_scores = last_outputs[value_leg]
            out["dump_outputs"] = {"leg": value_leg, **dump_outputs(args.dump_outputs, {"top_k_ids": top_ids, "top_k_scores": top_scores})}
        print(json.dumps(out), flush=True)
    if sharded:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
