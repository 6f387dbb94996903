"""GPU: the candidate-key kernels (rails_group_keys_pack / rails_group_keys_merge_own) against the torch restatement and a numpy uint64
sort, and ShardedMoLNaiveTopK / ShardedMoLCombTopK through the HIP modules in two processes -- one rank per GPU over nccl where two devices
are visible, both ranks on GPU 0 over gloo otherwise (the pattern of tests/test_generic_route_sharded_gpu.py; one spawn covers all cases).
Oracle of the global form: the single-device MoLNaiveTopK / MoLCombTopK over the whole corpus -- scores bit for bit, ids wherever the score
is above the duplicate mark -32767.0."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_sharded_gpu import _free_port

pytestmark = pytest.mark.gpu
DUP = -32767.0
POS_MASK = (1 << 48) - 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tie_scores(shape, g):
    s = (torch.randint(-8, 9, shape, generator=g).float() * 0.125).bfloat16().float()
    flat = s.view(-1)
    for j, v in enumerate((float("inf"), float("-inf"), -0.0, 0.0, float("nan"), -float("nan"))):
        if j < flat.numel():
            flat[(j * 7919) % flat.numel()] = v
    return s


def test_pack_equals_the_restatement_bit_for_bit(dev):
    from rails_amd import engine as E
    from rails_amd.sharded import pack_group_keys

    g = torch.Generator().manual_seed(3)
    for rows, kl, slots, offset, n_local in ((1, 1, 1, 0, 10), (577, 5, 5, 123_456_789_012, 1000), (2048, 100, 128, (1 << 48) - 5000, 5000),
                                            (64, 0, 7, 5, 0), (33, 128, 200, 1 << 33, 1 << 20)):
        s = _tie_scores((rows, kl), g)
        p = torch.randint(0, max(n_local, 1), (rows, kl), generator=g)
        if kl > 2:
            p[:, 1] = -1                                  # a hole packs as a pad
        got = E.group_keys_pack(s.to(dev), p.to(dev), offset, n_local, slots)
        assert torch.equal(got.cpu(), pack_group_keys(s, p, offset, slots, n_local)), (rows, kl, slots)
    with pytest.raises(ValueError, match="48 bits"):
        E.group_keys_pack(s.to(dev), p.to(dev), (1 << 48) - 10, 1 << 20, 200)


def _sorted_lists(R, rows, k, g, span=1000):
    """(R, rows, k) int64 key bit patterns: every list descending, ragged pads at its end, row 0 all pads; rank r owns [r * span, (r + 1) * span)"""
    from rails_amd.sharded import pack_group_keys

    out = np.zeros((R, rows, k), dtype=np.uint64)
    for r in range(R):
        s = _tie_scores((rows, k), g)
        p = torch.argsort(torch.rand((rows, span), generator=g), dim=1)[:, :k] if k <= span else torch.arange(k).repeat(rows, 1)
        keys = pack_group_keys(s, p, r * max(span, k), k).numpy().view(np.uint64)
        keys = np.sort(keys, axis=1)[:, ::-1].copy()
        keep = torch.randint(0, k + 1, (rows,), generator=g).numpy()
        keys[np.arange(k)[None, :] >= keep[:, None]] = 0
        keys[0] = 0
        out[r] = keys
    return out


def _merge_reference(keys, lo, hi):
    R, rows, k = keys.shape
    flat = np.ascontiguousarray(keys.transpose(1, 0, 2)).reshape(rows, R * k)
    best = np.sort(flat, axis=1)[:, ::-1][:, :k]
    gpos = (np.uint64(POS_MASK) - (best & np.uint64(POS_MASK))).astype(np.int64)
    gpos[best == 0] = -1
    local = np.where((gpos >= lo) & (gpos < hi), gpos - lo, -1)
    return gpos, local


@pytest.mark.parametrize("R", [1, 2, 8])
@pytest.mark.parametrize("k", [1, 5, 128])
def test_merge_own_equals_a_uint64_sort(dev, R, k):
    from rails_amd import engine as E

    g = torch.Generator().manual_seed(100 * R + k)
    span = max(1000, k)
    for rows in (1, 577, 2048):
        keys = _sorted_lists(R, rows, k, g, span)
        own = R // 2
        lo, hi = own * span, (own + 1) * span
        want_g, want_l = _merge_reference(keys, lo, hi)
        gathered = torch.from_numpy(keys.view(np.int64)).to(dev)
        local, gpos = E.group_keys_merge_own(gathered.view(-1), R, rows, k, lo, hi, want_global=True)
        assert np.array_equal(gpos.cpu().numpy(), want_g) and np.array_equal(local.cpu().numpy(), want_l), (R, k, rows)
        if rows > 1:
            assert bool((gpos[0] == -1).all()) and bool((local[0] == -1).all())          # the all-pad row
        # the strided union output: G key rows per union row behind a column offset, inside messages longer than these rows
        G = 4 if rows % 4 == 0 else 1
        col, tail = 3, 5
        msg = torch.full((R, rows * k + 11), -1, dtype=torch.int64, device=dev)
        msg[:, 4 : 4 + rows * k] = gathered.view(R, rows * k)
        union = torch.full((rows // G, col + G * k + tail), -7, dtype=torch.int64, device=dev)
        E.group_keys_merge_own(msg.view(-1)[4:], R, rows, k, lo, hi, out_local=union, out_col=col, rows_per_out_row=G, rank_stride=rows * k + 11)
        u = union.cpu().numpy()
        assert np.array_equal(u[:, col : col + G * k], want_l.reshape(rows // G, G * k))
        assert (u[:, :col] == -7).all() and (u[:, col + G * k :] == -7).all()             # nothing written outside the block
        # lists that are not descending take the in-LDS sort: same result
        if k > 1:
            perm = torch.randperm(k, generator=g)
            shuffled = gathered[:, :, perm].contiguous()
            local2, gpos2 = E.group_keys_merge_own(shuffled.view(-1), R, rows, k, lo, hi, want_global=True)
            assert np.array_equal(gpos2.cpu().numpy(), want_g) and np.array_equal(local2.cpu().numpy(), want_l)


def test_merge_own_refuses_what_does_not_fit(dev):
    from rails_amd import engine as E

    keys = torch.zeros(9 * 2048, dtype=torch.int64, device=dev)
    assert not E.group_keys_supported(9, 2048)
    with pytest.raises(NotImplementedError):
        E.group_keys_merge_own(keys, 9, 1, 2048, 0, 10)


# ---- two ranks through the HIP modules ------------------------------------------------------------------------------------------------
def _same_ranking(got, want, cols, what):
    """scores bit for bit; ids wherever the score is above the duplicate mark"""
    s, i = got
    ws, wi = want[0][:, :cols], want[1][:, :cols]
    assert s.shape == ws.shape and i.shape == wi.shape, (what, s.shape, ws.shape)
    assert torch.equal(s.view(torch.int32), ws.contiguous().view(torch.int32)), f"{what}: scores differ from the single-device ranking"
    scored = ws > DUP
    assert torch.equal(i[scored], wi[scored]), f"{what}: ids differ from the single-device ranking"


def _worker(rank: int, world: int, port: int, ret):
    import rails_amd
    from oracle import mol_oracle as O
    from rails_amd import engine as E
    from rails_amd.sharded import ShardedMoLCombTopK, ShardedMoLNaiveTopK, shard_bounds
    from tests.test_gpu_parity import build_module

    torch.set_num_threads(8)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    multi = torch.cuda.device_count() >= world
    dev = torch.device("cuda", rank if multi else 0)
    torch.cuda.set_device(dev)
    if multi:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        solo = [dist.new_group([r]) for r in range(world)][rank]          # a group of this rank alone (every rank creates every group)
        B = 9
        for name, methods in (("amzn-books", ("Naive5", "Comb5_200")), ("ml-20m", ("Naive5",))):
            cfg = O.CONFIGS[name]
            mol = build_module(cfg, O.synthetic_weights(cfg, seed=1), dev)
            G = cfg.query_dot_product_groups * cfg.item_dot_product_groups
            aux = {"user_ids": (torch.arange(B, dtype=torch.int64, device=dev) * 7 + 5)} if cfg.uid_embedding_hash_sizes else {}
            q = O.synthetic_queries(cfg, B, seed=5).to(dev)
            for n_items in (70_001, 331):
                X = torch.from_numpy(O.hash_item_table(7, 0, n_items, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
                ids = (torch.arange(n_items, dtype=torch.int64, device=dev) * 3 + 1).unsqueeze(0)
                lo, hi = shard_bounds(n_items, world, rank)
                for method in methods:
                    kg, kc = (5, 200) if method.startswith("Comb") else (5, 0)
                    W = G * kg + kc
                    k = 200

                    def single(x, i):
                        n = i.shape[1]
                        if kc:
                            return rails_amd.MoLCombTopK(mol, x, i, avg_top_k=min(kc, n), k_per_group=min(kg, n))
                        return rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=min(kg, n))

                    def sharded(x, i, n_total, **kw):
                        if kc:
                            return ShardedMoLCombTopK(mol, x, i, n_total, avg_top_k=kc, k_per_group=kg, **kw)
                        return ShardedMoLNaiveTopK(mol, x, i, n_total, k_per_group=kg, **kw)

                    what = f"{name} {method} n={n_items} rank {rank}"
                    with torch.inference_mode():
                        full = single(X, ids)(q, k=k, **aux)
                        assert full[0].shape[1] == W
                        # 2b: the global form == the single-device module over the whole corpus
                        sh = sharded(X[:, lo:hi], ids[:, lo:hi], n_items, global_candidates=True)
                        got = sh(q, k=k, **aux)
                        again = sh(q, k=k, **aux)
                        assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), what
                        _same_ranking(got, full, min(k, W), what + " global")
                        info = sh.exchange_info()
                        assert info["collectives_per_step"] == 2 and info["candidate_message_bytes"] == 8 * (B * G * kg + B * kc), info
                        assert sh.forward_filtered(q, k, ids[:, :61].expand(B, 61), 100, **aux) is None
                        ret[(rank, name, method, n_items)] = (dist.get_backend(), got[0].cpu(), got[1].cpu())
                        wide = sh(q, k=min(W + 50, n_items), **aux)          # more than the union holds: W columns, the masked tail included
                        if n_items >= W + 50:
                            _same_ranking(wide, full, W, what + " global, all columns")
                        # 2c: the fused scans on rank 0 only, the materialising path on rank 1
                        if n_items > 10_000:
                            mixed = sharded(X[:, lo:hi], ids[:, lo:hi], n_items, global_candidates=True)
                            local = mixed._local_module
                            local.fused_component_min_items = 1024 if rank == 0 else 1 << 40
                            if kc:
                                local.fused_coarse_min_items = 1024 if rank == 0 else 1 << 40
                            _same_ranking(mixed(q, k=k, **aux), full, min(k, W), what + " mixed scan paths")
                        # 2e: a NaN query row stays in its row
                        qn = q.clone()
                        qn[2] = float("nan")
                        bad = sh(qn, k=k, **aux)
                        keep = [b for b in range(B) if b != 2]
                        assert torch.equal(bad[0][keep], got[0][keep]) and torch.equal(bad[1][keep], got[1][keep]), what + " NaN row"
                        with pytest.raises(RuntimeError, match="out of range"):
                            sh(q, k=n_items + 1, **aux)
                        # 2d: the per-shard form == the merge of every shard's own single-device ranking
                        per = sharded(X[:, lo:hi], ids[:, lo:hi], n_items)
                        ps, pi = per(q, k=k, **aux)
                        cols = min(k, W)
                        parts_s, parts_i = [], []
                        for r in range(world):
                            a, b = shard_bounds(n_items, world, r)
                            s_r, i_r = single(X[:, a:b], ids[:, a:b])(q, k=k, **aux)
                            s_r, i_r = s_r[:, :cols].float(), i_r[:, :cols]
                            pad = cols - s_r.shape[1]
                            parts_s.append(torch.cat([s_r, s_r.new_full((B, pad), float("-inf"))], 1))
                            parts_i.append(torch.cat([i_r, i_r.new_full((B, pad), -1)], 1))
                        ws, wi = E.topk(torch.cat(parts_s, 1).contiguous(), cols, ids=torch.cat(parts_i, 1).contiguous())
                        assert torch.equal(ps, ws.to(ps.dtype)) and torch.equal(pi, wi), what + " per-shard"
                        assert per.exchange_info()["collectives_per_step"] == 1
                        kk = 90
                        inv = pi[:, torch.randperm(pi.shape[1], device=dev)[:61]]
                        cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
                        kp = min(kk + 61, n_items, W)
                        plain = per(q, k=kp, **aux)
                        want_i, want_s = E.filter_seen_ids(plain[1], plain[0], inv, kk)
                        c_i, c_s, _ = cand.get_top_k_outputs(q, kk, aux, per, inv, truncate_k_prime_to=kp)
                        assert torch.equal(c_i, want_i) and torch.equal(c_s, want_s), what + " get_top_k_outputs"
                        # one rank, the whole exchange path in a group of its own: both forms equal the single-device module
                        if n_items == 331 or method == "Naive5":
                            for glob in (False, True):
                                cls = type("OneRank", (ShardedMoLCombTopK if kc else ShardedMoLNaiveTopK,), {"EXCHANGE_WITH_ONE_RANK": True})
                                one = (cls(mol, X, ids, n_items, avg_top_k=kc, k_per_group=kg, global_candidates=glob, group=solo) if kc else
                                       cls(mol, X, ids, n_items, k_per_group=kg, global_candidates=glob, group=solo))
                                assert one._exchange and one._world == 1
                                _same_ranking(one(q, k=k, **aux), full, min(k, W), what + f" one rank, global={glob}")
            with pytest.raises(NotImplementedError, match="use_faiss"):
                ShardedMoLNaiveTopK(mol, X[:, lo:hi], ids[:, lo:hi], n_items, k_per_group=5, use_faiss=True)
    finally:
        dist.destroy_process_group()


def test_two_ranks_naive_and_comb():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    cases = [("amzn-books", "Naive5"), ("amzn-books", "Comb5_200"), ("ml-20m", "Naive5")]
    assert set(ret.keys()) == {(r, name, m, n) for r in range(world) for name, m in cases for n in (70_001, 331)}
    for name, m in cases:
        for n in (70_001, 331):
            a, b = ret[(0, name, m, n)], ret[(1, name, m, n)]
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (name, m, n)          # identical on every rank
            assert a[0] == ("nccl" if torch.cuda.device_count() >= world else "gloo")
