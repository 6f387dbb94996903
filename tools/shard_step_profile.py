#!/usr/bin/env python3
"""Per-rank step of the item-sharded path at world size R, emulated on ONE GPU: rank 0's shard of amzn-books, the real
prologue / scoring / local top-k / pack / merge / filter kernels, and the all-gather replaced by a device copy of the
rank's own message R times (so merge sees R*k' keys).  Everything but the RCCL latency is real: run it under
`rocprofv3 --kernel-trace --stats` to see the fixed per-step costs that bound strong scaling."""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rails_amd
from rails_amd import engine as E
from rails_amd.sharded import shard_bounds
from oracle import mol_oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--world", type=int, default=8)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--precision", default=None, help="fp32 (default) | f16x3 | f16x3-exact | f16-exact (the module's verified route, proved PER SHARD) | "
                                                 "proved-global (ShardedMoLBruteForceTopK's flow: one proof for all shards, its collectives replaced by copies)")
ap.add_argument("--method", default=None, help="Naive5 | Naive100 | Comb5_200 | Comb100_1000: the per-rank step of ShardedMoLNaiveTopK / ShardedMoLCombTopK "
                                              "instead (both forms), beside the single-device module on the whole corpus; medians of per-step event times")
ap.add_argument("--json", default=None, help="with --method: append the medians to this JSON file (a list of records)")
ap.add_argument("--pipeline", action="store_true", help="exchange (copy + merge + filter) of step i on a second stream, behind step i+1's scoring")
a = ap.parse_args()
dev = torch.device("cuda", 0)
cfg = O.CONFIGS["amzn-books"]
N, B, k, kp, width = 695762, 32, 120, 200, 61
w = O.synthetic_weights(cfg, seed=0)
mol, _ = rails_amd.create_mol_interaction_module(
    cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
    cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
    cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
    query_nonlinearity=cfg.query_nonlinearity, uid_embedding_hash_sizes=list(cfg.uid_embedding_hash_sizes) or None)
mol.load_state_dict(w, strict=True)
mol = mol.to(dev).eval()
if a.precision and a.precision != "proved-global":
    mol.precision = a.precision
lo, hi = shard_bounds(N, a.world, 0)
if a.method:
    # ---- the candidate generators: rank 0's step in both forms, collectives replaced by device copies (no RCCL latency) -----------------
    import json, re, statistics
    from rails_amd.sharded import ShardedMoLCombTopK, ShardedMoLNaiveTopK
    m = re.fullmatch(r"(Naive)(\d+)|(Comb)(\d+)_(\d+)", a.method)
    kg, kc = (int(m.group(2)), 0) if m.group(1) else (int(m.group(4)), int(m.group(5)))
    G = cfg.query_dot_product_groups * cfg.item_dot_product_groups
    W, R, n_loc = G * kg + kc, a.world, hi - lo
    Xall = torch.from_numpy(O.hash_item_table(1, 0, N, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
    ids_all = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
    q = O.synthetic_queries(cfg, B).to(dev)
    kk = min(kp, W)

    def module(x, i):
        if kc:
            return rails_amd.MoLCombTopK(mol, x, i, avg_top_k=kc, k_per_group=kg)
        return rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=kg)

    def median_ms(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    with torch.inference_mode():
        single = module(Xall, ids_all)
        t_single = median_ms(lambda: single(q, k=kk))
        del single
        local = module(Xall[:, lo:hi], ids_all[:, lo:hi])
        rows = B * G
        n_keys = rows * kg + B * kc
        shift = torch.arange(R, dtype=torch.int64, device=dev).view(R, 1) * n_loc       # rank r's copy names items r * n_loc further on

        def finish(s, i):
            gathered = E.pack_candidates(s, i, kk).repeat(R, 1)
            return E.merge_candidates(gathered, R, kk, kk)

        def per_shard():
            s, i = local(q, k=kk)
            return finish(s[:, :kk], i[:, :kk])

        def global_form():
            cand = local.local_candidates(q)
            msg = torch.empty(n_keys, dtype=torch.int64, device=dev)
            E.group_keys_pack(cand[0], cand[1], lo, n_loc, kg, out=msg[: rows * kg])
            if kc:
                E.group_keys_pack(cand[2], cand[3], lo, n_loc, kc, out=msg[rows * kg :])
            gathered = (msg.view(1, n_keys) - shift).contiguous()                         # stands for the all-gather
            union = torch.empty((B, W), dtype=torch.int64, device=dev)
            for first, n_rows, kx, col, per_row in ((0, rows, kg, 0, G), (rows * kg, B, kc, G * kg, 1)):
                if kx:
                    E.group_keys_merge_own(gathered.view(-1)[first:], R, n_rows, kx, lo, hi, out_local=union, out_col=col, rows_per_out_row=per_row,
                                           rank_stride=n_keys)
            return finish(*local.rerank_union_masked(q, union, kk))

        t_per, t_glob = median_ms(per_shard), median_ms(global_form)
    rec = {"method": a.method, "world": R, "shard_items": n_loc, "batch": B, "k": kk, "union_width": W, "steps": a.steps,
           "single_device_whole_corpus_ms": round(t_single, 4), "per_shard_form_ms": round(t_per, 4), "global_form_ms": round(t_glob, 4),
           "candidate_message_bytes": 8 * n_keys, "note": "rank 0's step on one GPU, collectives replaced by device copies (no RCCL latency); medians"}
    print(json.dumps(rec))
    if a.json:
        old = json.load(open(a.json)) if os.path.exists(a.json) else []
        json.dump(old + [rec], open(a.json, "w"), indent=1)
    sys.exit(0)
X = torch.from_numpy(O.hash_item_table(1, lo, hi - lo, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
ids = torch.arange(lo + 1, hi + 1, dtype=torch.int64, device=dev).unsqueeze(0)
q = O.synthetic_queries(cfg, B).to(dev)
inv = torch.zeros((B, width), dtype=torch.int64, device=dev)
with torch.inference_mode():
    tk = rails_amd.MoLBruteForceTopK(mol, X, ids, exact_mode="dense")     # "fp32" = the dense fp32 kernels (the module's default is the proved mode)
    eng = tk._bind()
    logits = torch.empty((B, hi - lo), dtype=torch.float32, device=dev)

    tk.SPECULATE_MIN_ITEMS = 0
    side = torch.cuda.Stream(dev)

    if a.precision == "proved-global":
        del tk
        rails_amd.MoLBruteForceTopK.SPECULATE_MIN_ITEMS = 0
        tk = rails_amd.MoLBruteForceTopK(mol, X, ids, exact_mode="proved")
        assert tk.shard_can_speculate()
        eps, state = tk._proved_eps(), torch.zeros(8, dtype=torch.float32, device=dev)
        total = kp + max(824, 3 * kp)
        per = -(-total // a.world)
        kc = min((per + int(4 * per ** 0.5) + 32 + 31) // 32 * 32, hi - lo)
        print("global proof: eps", eps, "kc per rank", kc)

    host = torch.zeros(8, dtype=torch.float32).pin_memory()
    call_ws = torch.zeros(8 + 4 * B, dtype=torch.int32, device=dev)
    issued = [0]

    def global_step():
        # round 6: one message (top-k' | ids | m | err), one exchange, merge + verdict + filter in one launch, the verdict read from the pinned mirror
        msg, qp32 = tk.speculate_for_shard(q, kp, kc)
        sp = tk._engine.spec
        off = (B + 32 // sp.query_dot_product_groups - 1) // (32 // sp.query_dot_product_groups) * 32 * sp.dot_product_dimension
        gq = qp32[off : off + B * sp.num_logits]
        gathered = msg.repeat(a.world, 1)                                   # stands for the all-gather
        out = E.merge_candidates_verdict(gathered, a.world, kp, kp, eps, 1.0, gq, sp.num_logits, tk._gate_guard_limit, state, host, call_ws, (inv, k))
        issued[0] += 1
        if not a.pipeline:
            while float(host[5]) < issued[0]:
                pass
            assert int(host.view(torch.int32)[1]) == 0, "the emulated global verdict failed"
        return out

    def local_part():
        if a.precision == "proved-global":
            return None
        if a.precision and a.precision.endswith("-exact"):
            s, top = tk(q, k=min(kp, hi - lo))
        else:
            qpack, _, _ = eng.query_pack(q, None)
            eng.score_dense(qpack, B, tk._index, out=logits)
            s, top = E.topk(logits, min(kp, hi - lo), ids=tk._ids_flat)
        return E.pack_candidates(s, top, kp) if a.world > 1 else (s, top)

    def exchange(msg):
        if a.precision == "proved-global":
            return global_step()
        if a.world > 1:
            gathered = msg.repeat(a.world, 1)
            if E.merge_filter_fusable(kp, inv.shape[1], k):   # the sharded module's route: the seen-id filter inside the merge launch
                return E.merge_candidates_filtered(gathered, a.world, kp, kp, inv, k)
            s, top = E.merge_candidates(gathered, a.world, kp, kp)
        else:
            s, top = msg
        return E.filter_seen_ids(top, s, inv, k)

    def run(n):
        if not a.pipeline:
            for _ in range(n):
                exchange(local_part())
            return
        cur = torch.cuda.current_stream(dev)
        msg = local_part()
        for i in range(n):
            ev = torch.cuda.Event(); ev.record()
            nxt = local_part() if i + 1 < n else None
            side.wait_event(ev)
            with torch.cuda.stream(side):
                exchange(msg)
            msg = nxt
        cur.wait_stream(side)

    run(5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(a.steps)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
if a.precision == "proved-global":
    print("verdict state [seen err, redo, eps, err, gap, calls, redone, guard max]:", state.view(torch.float32).tolist(), "redo flag", int(state.view(torch.int32)[1]))
print(f"world={a.world} shard={hi - lo} items precision={a.precision or 'fp32'} pipeline={a.pipeline}: {dt * 1e3:.3f} ms/step (no RCCL latency) -> {B / dt:.0f} q/s if all ranks match")
