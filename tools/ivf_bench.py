#!/usr/bin/env python3
"""MoLNaiveTopK(use_faiss=True) -- the native IVF-Flat candidate generator -- on synthetic amzn-books 8x8x32 (N = 695 762), with the
algorithms_bench.py timing protocol (3 warm-ups + 20 timed get_top_k_outputs calls, k = 120, k' = 200, device sync):
index build time, list-size imbalance, ms per call for B in {1, 8, 32} x nprobe in {1, 4, 16} next to MoLNaiveTopK5 at the same B,
and overlap@10 / @120 with MoLNaiveTopK5 and MoLBruteForceTopK.  Prints one JSON document.
  python tools/ivf_bench.py [--batches 1,8,32] [--nprobes 1,4,16]
--filtered: the filtered-lists leg instead (MoLNaiveTopK(use_faiss=True, filtered_lists=True)): B in {1, 8, 32} x
nprobe in {1, 4}, the same protocol, ms per call with nothing hidden and no tags (the plain search of the same module, in the same run),
with a random 10 % / 50 % of the corpus hidden, and with per-row allowed_tags keeping 10 % / 1 % (ten distinct words cycled over the
rows).  Writes profiles/ivf_filtered.json.
"""
import argparse
import gc, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, rails_amd
from oracle import mol_oracle as O   # input generators only

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8,32")
ap.add_argument("--nprobes", default="1,4,16")
ap.add_argument("--nlist", type=int, default=100)
ap.add_argument("--filtered", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
cfg_key, N, width = bench.WORKLOADS["amzn-books"]
cfg = O.CONFIGS[cfg_key]
k, kp, kg = 120, 200, 5
mol, _ = rails_amd.create_mol_interaction_module(
    cfg.query_embedding_dim, cfg.item_embedding_dim, cfg.dot_product_dimension, cfg.query_dot_product_groups,
    cfg.item_dot_product_groups, cfg.temperature, 0.0, cfg.query_hidden_dim, 0.1, cfg.item_hidden_dim,
    cfg.gating_query_hidden_dim, cfg.gating_qi_hidden_dim, cfg.gating_item_hidden_dim, cfg.softmax_dropout_rate, False,
    query_nonlinearity=cfg.query_nonlinearity)
mol.load_state_dict(O.synthetic_weights(cfg, seed=0), strict=True)
mol = mol.to(dev).eval()
X = torch.from_numpy(O.hash_item_table(1, 0, N, cfg.item_embedding_dim)).to(dev).unsqueeze(0)
ids = torch.arange(1, N + 1, dtype=torch.int64, device=dev).unsqueeze(0)
model = type("M", (), {"_ndp_module": mol})()
cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)


def timed(tk, q, inv, aux=None):
    aux = aux or {}
    for _ in range(3):
        out_ids, _, _ = cand.get_top_k_outputs(q, k, aux, tk, inv, truncate_k_prime_to=kp)
    torch.cuda.synchronize()
    gc.collect()
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        out_ids, _, _ = cand.get_top_k_outputs(q, k, aux, tk, inv, truncate_k_prime_to=kp)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out_ids.cpu(), {"ms_avg": sum(ts) / len(ts), "ms_min": min(ts), "ms_median": sorted(ts)[len(ts) // 2]}


def overlap(x, y, kk):
    return sum(len(set(r.tolist()) & set(s.tolist())) for r, s in zip(x[:, :kk], y[:, :kk])) / (x.shape[0] * kk)


def filtered_leg():
    """Every cell beside the same module's unfiltered call of the same (B, nprobe), timed in the same run."""
    doc = {"workload": f"amzn-books {cfg.query_dot_product_groups}x{cfg.item_dot_product_groups}x{cfg.dot_product_dimension}, N={N}, k={k}, k'={kp}, "
                       f"k_per_group={kg}, nlist={a.nlist}, MoLNaiveTopK(use_faiss=True, filtered_lists=True)",
           "protocol": "3 warm-ups + 20 timed get_top_k_outputs calls, wall clock with device sync (tools/algorithms_bench.py)",
           "tags": "bits 0-9 each on a random 10 % of the items, bits 10-19 each on a random 1 %; row b of a batch allows bit (b % 10) of the fraction's ten",
           "rows": []}
    gen = torch.Generator().manual_seed(7)
    tags = torch.zeros(N, dtype=torch.int64)
    for bit in range(20):
        tags[torch.randperm(N, generator=gen)[: N // (10 if bit < 10 else 100)]] |= 1 << bit
    order = torch.randperm(N, generator=gen)
    with torch.inference_mode():
        tk = rails_amd.MoLNaiveTopK(mol, X, ids, k_per_group=kg, use_faiss=True, nlist=a.nlist, filtered_lists=True)
        tk.ivf_index()
        tk.set_item_tags(tags.to(dev))
        for B in (1, 8, 32):
            q = O.synthetic_queries(cfg, B).to(dev)
            inv = torch.zeros((B, width), dtype=torch.int64, device=dev)
            for p in (1, 4):
                tk.nprobe = p
                row = {"B": B, "nprobe": p, "unfiltered": timed(tk, q, inv)[1]}
                for share in (10, 50):
                    hide = order[: N * share // 100]
                    tk.hide_items(hide)
                    row[f"hidden_{share}pct"] = timed(tk, q, inv)[1]
                    tk.unhide_items(hide)
                for share, first in ((10, 0), (1, 10)):
                    words = [1 << (first + b % 10) for b in range(B)]
                    row[f"tags_per_row_{share}pct"] = timed(tk, q, inv, {"allowed_tags": words})[1]
                doc["rows"].append(row)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ivf_filtered.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


gc.disable()
if a.filtered:
    filtered_leg()
    sys.exit(0)
out = {"workload": f"amzn-books {cfg.query_dot_product_groups}x{cfg.item_dot_product_groups}x{cfg.dot_product_dimension}, N={N}, k={k}, k'={kp}, "
                   f"k_per_group={kg}, nlist={a.nlist}",
       "protocol": "3 warm-ups + 20 timed get_top_k_outputs calls, wall clock with device sync (tools/algorithms_bench.py)",
       "weights": "random-init, synthetic items (overlap with brute force is NOT the trained-model recall)", "rows": []}
with torch.inference_mode():
    ivf_mod = rails_amd.MoLNaiveTopK(mol, X, ids, k_per_group=kg, use_faiss=True, nlist=a.nlist)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ivf = ivf_mod.ivf_index()
    torch.cuda.synchronize()
    out["build_s"] = time.perf_counter() - t0
    sizes = ivf.list_sizes().double()
    out["list_size"] = {"min": int(sizes.min()), "max": int(sizes.max()), "mean": float(sizes.mean()),
                        "max_over_mean": float((sizes.max(dim=1).values / sizes.mean(dim=1)).max()),
                        "imbalance_sum_sq": float(((sizes ** 2).sum(dim=1) * a.nlist / N ** 2).max())}   # 1.0 = equal lists; FAISS's imbalance factor
    naive = rails_amd.get_top_k_module("MoLNaiveTopK5", model, X, ids)
    brute = rails_amd.get_top_k_module("MoLBruteForceTopK", model, X, ids)
    bytes_per_item = cfg.dot_product_dimension * 2 + 4
    for B in [int(b) for b in a.batches.split(",")]:
        q = O.synthetic_queries(cfg, B).to(dev)
        inv = torch.zeros((B, width), dtype=torch.int64, device=dev)
        ex_ids, t_brute = timed(brute, q, inv)
        nv_ids, t_naive = timed(naive, q, inv)
        _, eq, _ = ivf_mod._bind().query_pack(q, None, want_plain=True)
        cs = torch.einsum("bid,mld->biml", eq.double(), ivf.centroids.double())      # (B, P_Q, P_X, nlist)
        for p in [int(x) for x in a.nprobes.split(",")]:
            ivf_mod.nprobe = p
            iv_ids, t_ivf = timed(ivf_mod, q, inv)
            probed = torch.topk(cs, p, dim=3).indices                                                   # distinct (group, list) pairs probed
            pairs = torch.unique(torch.arange(cfg.item_dot_product_groups, device=dev).view(1, 1, -1, 1) * a.nlist + probed)
            probed_bytes = int(sizes.flatten().to(dev)[pairs].sum()) * bytes_per_item
            out["rows"].append({"B": B, "nprobe": p, "ivf": t_ivf, "MoLNaiveTopK5": t_naive, "MoLBruteForceTopK": t_brute,
                                "ivf_over_naive5": t_ivf["ms_avg"] / t_naive["ms_avg"], "distinct_probed_lists": int(pairs.numel()),
                                "distinct_probed_list_bytes": probed_bytes,
                                "overlap_naive5@10": overlap(iv_ids, nv_ids, 10), "overlap_naive5@120": overlap(iv_ids, nv_ids, 120),
                                "overlap_brute@10": overlap(iv_ids, ex_ids, 10), "overlap_brute@120": overlap(iv_ids, ex_ids, 120)})
        ivf_mod.nprobe = 1
print(json.dumps(out, indent=1))
