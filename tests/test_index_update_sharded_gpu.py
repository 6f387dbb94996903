"""GPU: update_items on the item-sharded modules, two processes (one rank per GPU over nccl where two devices are visible, both ranks on
GPU 0 over gloo otherwise: the pattern of tests/test_sharded_candidates_gpu.py).  Oracle: the single-device module built from the updated
table, bit for bit; append_items refuses on every rank."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_sharded_gpu import _free_port

pytestmark = pytest.mark.gpu
DUP = -32767.0


def _worker(rank: int, world: int, port: int, ret):
    import rails_amd
    from oracle import mol_oracle as O
    from rails_amd.sharded import ShardedMoLBruteForceTopK, ShardedMoLNaiveTopK, shard_bounds
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
        cfg = O.CONFIGS["amzn-books"]
        mol = build_module(cfg, O.synthetic_weights(cfg, seed=1), dev)
        n, B, k = 70_001, 32, 100
        q = O.synthetic_queries(cfg, B, seed=5).to(dev)
        lo, hi = shard_bounds(n, world, rank)
        split = shard_bounds(n, world, 0)[1]
        g = torch.Generator().manual_seed(17)           # the same draw on every rank
        pos = torch.unique(torch.cat([torch.tensor([0, n - 1, split - 1, split, 31, 32]), torch.randint(0, n, (300,), generator=g)]))
        pos = pos[torch.randperm(pos.numel(), generator=g)]
        with torch.inference_mode():
            for name in ("brute", "naive"):
                X = torch.from_numpy(O.hash_item_table(7, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
                ids = (torch.arange(n, dtype=torch.int64, device=dev) * 3 + 1).unsqueeze(0)
                if name == "brute":
                    sh = ShardedMoLBruteForceTopK(mol, X[:, lo:hi].clone(), ids[:, lo:hi].clone(), n)
                    single = lambda x, i: rails_amd.MoLBruteForceTopK(mol, x, i)       # noqa: E731
                else:
                    sh = ShardedMoLNaiveTopK(mol, X[:, lo:hi].clone(), ids[:, lo:hi].clone(), n, k_per_group=5, global_candidates=True)
                    single = lambda x, i: rails_amd.MoLNaiveTopK(mol, x, i, k_per_group=5)   # noqa: E731
                before = sh(q, k=k)
                best = (before[1][:, 0] - 1) // 3
                rows = torch.from_numpy(O.hash_item_table(23, 10_000_000, pos.numel(), cfg.item_embedding_dim)).to(dev)
                rows[:4] = X[0, best[:4]]                   # copies of some queries' best items: the updated positions enter the results
                new_ids = ids[0, pos.to(dev)] + 1_000_000_007
                sh.update_items(pos, rows, new_ids)
                X[0, pos.to(dev)], ids[0, pos.to(dev)] = rows, new_ids
                want = single(X, ids)(q, k=k)
                got = sh(q, k=k)
                cols = got[0].shape[1]
                assert torch.equal(got[0].view(torch.int32), want[0][:, :cols].contiguous().view(torch.int32)), f"{name} rank {rank}: scores"
                scored = want[0][:, :cols] > DUP
                assert torch.equal(got[1][scored], want[1][:, :cols][scored]), f"{name} rank {rank}: ids"
                assert not torch.equal(before[1], got[1]) and bool((got[1] > 1_000_000_000).any()), f"{name}: the update changed nothing"
                with pytest.raises(NotImplementedError, match="shard bounds"):
                    sh.append_items(rows, new_ids)
                with pytest.raises(ValueError):
                    sh.update_items(torch.tensor([1, 1]), rows[:2])
                with pytest.raises(ValueError):
                    sh.update_items(torch.tensor([1, n]), rows[:2])
                ret[(rank, name)] = (got[0].cpu(), got[1].cpu())
    finally:
        dist.destroy_process_group()


def test_two_ranks_update_items():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert set(ret.keys()) == {(r, name) for r in range(world) for name in ("brute", "naive")}
    for name in ("brute", "naive"):
        a, b = ret[(0, name)], ret[(1, name)]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name            # identical on every rank
