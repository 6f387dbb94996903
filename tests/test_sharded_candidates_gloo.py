"""CPU, gloo, world_size 2: the collective logic of ShardedMoLNaiveTopK / ShardedMoLCombTopK (rails_amd/sharded.py) with the oracle standing in
for the HIP scans and rerank, and the torch restatement of the candidate keys (pack_group_keys / unpack_group_keys / merge_group_keys_own)
standing in for rails_group_keys_* (tests/test_sharded_candidates_gpu.py pins the kernels to this restatement bit for bit).
Global form == component_candidate_scores + per-row top-k_g + union_rerank over the WHOLE corpus; per-shard form == the merge of every
shard's own oracle result."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import mol_oracle as O
from rails_amd.sharded import (ShardedMoLCombTopK, ShardedMoLNaiveTopK, merge_group_keys_own, pack_group_keys, shard_bounds,
                               unpack_group_keys)
from tests.test_sharded_gloo import _free_port

DUP = -32767.0


def _bf16_scores_with_ties(rows, n, seed):
    g = torch.Generator().manual_seed(seed)
    s = (torch.randint(-6, 7, (rows, n), generator=g).float() * 0.25).bfloat16().float()      # few distinct values: heavy ties
    s[0, 0], s[0, 1], s[1, 2], s[1, 3] = float("inf"), float("-inf"), -0.0, 0.0
    return s, g


def test_key_order_is_score_descending_then_position_ascending():
    rows, n = 6, 300
    s, g = _bf16_scores_with_ties(rows, n, 0)
    pos = torch.stack([torch.randperm(5000, generator=g)[:n] for _ in range(rows)])
    keys = pack_group_keys(s, pos, 1 << 40, n)
    u = keys.numpy().view(np.uint64)
    for r in range(rows):
        got = np.argsort(u[r], kind="stable")[::-1]                         # descending unsigned keys (distinct: positions are)
        # -0.0 ranks below +0.0 (rails_topk's bit-pattern order): break Python's -0.0 == 0.0 tie the same way
        want = sorted(range(n), key=lambda j: (-s[r, j].item(), 1 if (s[r, j].item() == 0.0 and np.signbit(s[r, j].item())) else 0, pos[r, j].item()))
        assert list(got) == want
    sc, gp = unpack_group_keys(keys)
    assert torch.equal(sc.view(torch.int32), s.view(torch.int32)) and torch.equal(gp, pos + (1 << 40))


def test_pads_and_the_position_limit():
    s, _ = _bf16_scores_with_ties(3, 4, 1)
    pos = torch.tensor([[0, 1, 2, 3], [3, -1, 1, 0], [7, 6, 5, 4]])
    keys = pack_group_keys(s, pos, 100, 7)
    assert keys.shape == (3, 7) and bool((keys[:, 4:] == 0).all()) and int(keys[1, 1]) == 0          # short rows and holes pad with key 0
    assert bool((keys[:, :4][pos >= 0] != 0).all())
    sc, gp = unpack_group_keys(keys)
    assert bool((gp[:, 4:] == -1).all()) and int(gp[1, 1]) == -1 and bool(torch.isnan(sc[:, 4:]).all())
    # the last position that fits, and the first that does not
    top = pack_group_keys(s[:1, :1], torch.tensor([[5]]), (1 << 48) - 6, 1, n_local=6)
    assert int(unpack_group_keys(top)[1]) == (1 << 48) - 1
    with pytest.raises(ValueError, match="48 bits"):
        pack_group_keys(s[:1, :1], torch.tensor([[5]]), (1 << 48) - 5, 1, n_local=6)
    with pytest.raises(ValueError, match="48 bits"):
        pack_group_keys(s[:1, :1], torch.tensor([[0]]), -1, 1)
    # merge: the best k of R lists, pads last, ownership by range
    a = pack_group_keys(torch.tensor([[2.0, 1.0, 1.0]]), torch.tensor([[4, 0, 9]]), 0, 3)
    b = pack_group_keys(torch.tensor([[2.0, 1.0]]), torch.tensor([[0, 1]]), 10, 3)
    gpos, local = merge_group_keys_own(torch.stack([a, b]), 10, 20)
    assert gpos.tolist() == [[4, 10, 0]] and local.tolist() == [[-1, 0, -1]]
    gpos, _ = merge_group_keys_own(torch.stack([torch.zeros_like(a), torch.zeros_like(a)]), 0, 5)
    assert gpos.tolist() == [[-1, -1, -1]]


def _uids(cfg, B=3):
    return torch.arange(B, dtype=torch.int64) * 7 + 5 if cfg.uid_embedding_hash_sizes else None


def _coarse(cfg, w, q, X):
    return O.avg_topk_coarse_scores(cfg, w, q, X, _uids(cfg)).float()


def _group_scores(cfg, w, q, X):
    c = O.component_candidate_scores(cfg, w, q, X, _uids(cfg)).float()
    return c.reshape(-1, c.shape[-1])


def _expected_global(cfg, w, q, X, ids, kg, kc):
    """the single-device algorithm over the whole corpus, deterministic tie rule at the candidate selections"""
    B = q.shape[0]
    _, gp = O.select_topk_deterministic(_group_scores(cfg, w, q, X), kg)
    union = gp.reshape(B, -1)
    if kc:
        union = torch.cat([union, O.select_topk_deterministic(_coarse(cfg, w, q, X), kc)[1]], 1)
    return O.union_rerank(cfg, w, q, X, ids, torch.sort(union, dim=1).values, _uids(cfg))


def _worker(rank, world, port, case, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        name, n_items, kg, kc, k, split = case
        cfg = O.CONFIGS[name]
        w = O.synthetic_weights(cfg, seed=0)
        q = O.synthetic_queries(cfg, 3)
        G = cfg.query_dot_product_groups * cfg.item_dot_product_groups
        lo, hi = split[rank] if split is not None else shard_bounds(n_items, world, rank)
        X = torch.from_numpy(O.hash_item_table(1, lo, hi - lo, cfg.item_embedding_dim)).unsqueeze(0)
        ids = (torch.arange(lo, hi, dtype=torch.int64) * 3 + 1).unsqueeze(0)
        n = hi - lo

        def candidates_local(qq, **kw):
            gs, gp = O.select_topk_deterministic(_group_scores(cfg, w, qq, X), min(kg, n))
            if not kc:
                return gs, gp
            cs, cp = O.select_topk_deterministic(_coarse(cfg, w, qq, X), min(kc, n))
            return gs, gp, cs, cp

        def rerank_local(qq, union, kk, **kw):       # MoL on the union with holes; duplicates among owned positions masked
            idx = torch.sort(union, dim=1).values
            hole = idx < 0
            safe = idx.clamp_min(0)
            sc = O.mol_stages(cfg, w, qq, X.squeeze(0)[safe], kw.get("user_ids"))["logits"]
            dup = torch.cat([torch.zeros_like(idx[:, :1], dtype=torch.bool), idx[:, 1:] == idx[:, :-1]], 1)
            sc = torch.where(dup, torch.full_like(sc, DUP), sc)
            sc = torch.where(hole, torch.full_like(sc, float("-inf")), sc)
            cid = torch.where(hole, torch.full_like(idx, -1), ids.reshape(-1)[safe])
            s, p = O.select_topk_deterministic(sc, min(kk, idx.shape[1]))
            return s, torch.gather(cid, 1, p)

        def merge(scores, all_ids, kk):
            s, pos = O.select_topk_deterministic(scores, kk)
            return s, torch.gather(all_ids, 1, pos)

        def local_topk(qq, kk, **kw):               # the per-shard form: the oracle's single-device module on this shard
            s, i = _expected_global(cfg, w, qq, X, ids, min(kg, n), min(kc, n))
            return s[:, :kk], i[:, :kk]

        common = dict(candidates_local=candidates_local, rerank_local=rerank_local, merge=merge, groups=G,
                      shard_offset=lo if split is not None else None)
        make = (lambda **kw: ShardedMoLCombTopK(None, None, ids, n_items, avg_top_k=kc, k_per_group=kg, **kw)) if kc else \
               (lambda **kw: ShardedMoLNaiveTopK(None, None, ids, n_items, k_per_group=kg, **kw))
        glob = make(global_candidates=True, **common)
        aux = {"user_ids": _uids(cfg)} if cfg.uid_embedding_hash_sizes else {}
        s, i = glob(q, k=k, **aux)
        s2, i2 = glob(q, k=k, **aux)
        assert torch.equal(s, s2) and torch.equal(i, i2)
        info = glob.exchange_info()
        assert info["collectives_per_step"] == 2 and info["candidate_message_bytes"] == 8 * (3 * G * kg + 3 * kc)
        assert glob.forward_filtered(q, k, torch.zeros((3, 4), dtype=torch.int64), 2) is None
        with pytest.raises(RuntimeError, match="out of range"):
            glob(q, k=n_items + 1)
        per = make(local_topk=local_topk, merge=merge, groups=G)
        ps, pi = per(q, k=k, **aux)
        assert per.exchange_info()["collectives_per_step"] == 1
        cols = min(k, G * kg + kc)
        ls, li = (local_topk(q, min(cols, n)) if n > 0 else (torch.empty((3, 0)), torch.empty((3, 0), dtype=torch.int64)))
        ret[rank] = tuple(t.clone() for t in (s, i, ps, pi, ls, li))
    finally:
        dist.destroy_process_group()


CASES = [
    ("amzn-books", 300, 3, 0, 40, None),                       # Naive, c3 shape
    ("amzn-books", 300, 2, 25, 60, None),                      # Comb
    ("ml-20m", 600, 4, 0, 500, None),                          # c1 shape; k beyond the union width: W = 128 columns come back
    ("ml-20m", 200, 3, 10, 30, ((0, 0), (0, 200))),            # an empty shard (rank 0)
    ("amzn-books", 150, 5, 7, 50, ((0, 3), (3, 150))),         # a shard with fewer than k_g (and K') items
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-n{c[1]}-kg{c[2]}-K{c[3]}-{'split' if c[5] else 'even'}")
def test_sharded_candidate_modules_on_gloo(case):
    world = 2
    name, n_items, kg, kc, k, split = case
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), case, ret), nprocs=world, join=True)
    cfg = O.CONFIGS[name]
    w = O.synthetic_weights(cfg, seed=0)
    q = O.synthetic_queries(cfg, 3)
    X = torch.from_numpy(O.hash_item_table(1, 0, n_items, cfg.item_embedding_dim)).unsqueeze(0)
    ids = torch.arange(0, n_items, dtype=torch.int64) * 3 + 1
    es, ei = _expected_global(cfg, w, q, X, ids, kg, kc)
    W = cfg.query_dot_product_groups * cfg.item_dot_product_groups * kg + kc
    cols = min(k, W)
    # per-shard form: the merge (score desc, rank-major column asc) of every shard's own ranking, cut to its first k columns
    all_s = torch.cat([torch.cat([ret[r][4], torch.full((3, cols - ret[r][4].shape[1]), float("-inf"))], 1) for r in range(world)], 1)
    all_i = torch.cat([torch.cat([ret[r][5], torch.full((3, cols - ret[r][5].shape[1]), -1, dtype=torch.int64)], 1) for r in range(world)], 1)
    ms, mp_ = O.select_topk_deterministic(all_s, cols)
    for rank in range(world):
        s, i, ps, pi = ret[rank][:4]
        assert s.shape == (3, cols) and i.shape == (3, cols)
        assert torch.allclose(s, es[:, :cols], atol=1e-6, rtol=0)
        scored = es[:, :cols] > DUP
        assert torch.equal(i[scored], ei[:, :cols][scored])
        assert torch.equal(ps, ms) and torch.equal(pi, torch.gather(all_i, 1, mp_))
