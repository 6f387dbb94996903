"""GPU, two processes: ShardedMoLBruteForceTopK on a MoL shape that only the generic scoring route runs (4x4x64), in the style of
tests/test_sharded_gpu.py -- one rank per GPU over nccl where two devices are visible, both ranks on GPU 0 over gloo otherwise.
Oracle: the single-device MoLBruteForceTopK over the whole corpus, which every rank's result must equal bit for bit."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_sharded_gpu import _free_port

pytestmark = pytest.mark.gpu


def _worker(rank: int, world: int, port: int, sizes, ret):
    import rails_amd
    from oracle import mol_oracle as O
    from rails_amd import engine as E
    from rails_amd.sharded import ShardedMoLBruteForceTopK, shard_bounds
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
        cfg = O.MoLConfig(64, 64, 64, 4, 4)
        mol = build_module(cfg, O.synthetic_weights(cfg, seed=1), dev)
        assert mol.engine().route == "generic"
        for n_items in sizes:
            B, k = 9, 200
            q = O.synthetic_queries(cfg, B, seed=5).to(dev)
            X = torch.from_numpy(O.hash_item_table(7, 0, n_items, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
            ids = (torch.arange(n_items, dtype=torch.int64, device=dev) * 3 + 1).unsqueeze(0)
            lo, hi = shard_bounds(n_items, world, rank)
            with torch.inference_mode():
                sh = ShardedMoLBruteForceTopK(mol, X[:, lo:hi], ids[:, lo:hi], n_items)
                s, i = sh(q, k=k)
                s2, i2 = sh(q, k=k)   # second call: recycled buffers
                full_s, full_i = rails_amd.MoLBruteForceTopK(mol, X, ids)(q, k=k)
                assert torch.equal(s, s2) and torch.equal(i, i2)
                assert torch.equal(s, full_s) and torch.equal(i, full_i), "sharded exact top-k differs from the single-device result"
                assert not sh._global_proof(q) and sh._local_module._bind().route == "generic"      # the per-shard dense path on every rank
                q2 = O.synthetic_queries(cfg, B, seed=6).to(dev)
                h1, h2 = sh.submit(q, k), sh.submit(q2, k)
                p1, p2 = sh.result(h1), sh.result(h2)
                r2 = sh(q2, k=k)
                assert torch.equal(p1[0], s) and torch.equal(p1[1], i) and torch.equal(p2[0], r2[0]) and torch.equal(p2[1], r2[1]), "pipelined != unpipelined"
                kk = min(120, i.shape[1])
                inv = i[:, torch.randperm(i.shape[1], device=dev)[:61]]
                want_i, want_s = E.filter_seen_ids(i, s, inv, kk)
                cand = rails_amd.CandidateIndex(ids=ids, embeddings=X)
                c_i, c_s, _ = cand.get_top_k_outputs(q, kk, {}, sh, inv, truncate_k_prime_to=min(k, n_items))
                assert torch.equal(c_i, want_i) and torch.equal(c_s, want_s)
            ret[(rank, n_items)] = (dist.get_backend(), s.cpu(), i.cpu())
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_a_generic_shape():
    world, sizes = 2, (70_001, 331)      # second case: the last shard is shorter than k
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), sizes, ret), nprocs=world, join=True)
    assert set(ret.keys()) == {(r, n) for r in range(world) for n in sizes}
    for n in sizes:
        assert torch.equal(ret[(0, n)][1], ret[(1, n)][1]) and torch.equal(ret[(0, n)][2], ret[(1, n)][2])   # identical on every rank
        assert ret[(0, n)][0] == ("nccl" if torch.cuda.device_count() >= world else "gloo")
