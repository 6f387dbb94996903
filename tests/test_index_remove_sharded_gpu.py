"""GPU: remove_items on the item-sharded modules, two processes (the form of tests/test_index_update_sharded_gpu.py: one rank per GPU over nccl
where two devices are visible, both ranks on GPU 0 over gloo otherwise).  Removing items would move the shard bounds: every rank refuses, and the
wrapper answers afterwards as it did before."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_sharded_gpu import _free_port

pytestmark = pytest.mark.gpu


def _worker(rank: int, world: int, port: int, ret):
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
        with torch.inference_mode():
            for name in ("brute", "naive"):
                X = torch.from_numpy(O.hash_item_table(7, 0, n, cfg.item_embedding_dim)).unsqueeze(0).to(dev)
                ids = (torch.arange(n, dtype=torch.int64, device=dev) * 3 + 1).unsqueeze(0)
                if name == "brute":
                    sh = ShardedMoLBruteForceTopK(mol, X[:, lo:hi].clone(), ids[:, lo:hi].clone(), n)
                else:
                    sh = ShardedMoLNaiveTopK(mol, X[:, lo:hi].clone(), ids[:, lo:hi].clone(), n, k_per_group=5, global_candidates=True)
                before = sh(q, k=k)
                for pos in (torch.tensor([0, 5, n - 1]), torch.tensor([lo, hi - 1], device=dev), torch.empty(0, dtype=torch.int64)):
                    with pytest.raises(NotImplementedError, match="shard bounds"):
                        sh.remove_items(pos)
                got = sh(q, k=k)
                assert torch.equal(got[0].view(torch.int32), before[0].view(torch.int32)) and torch.equal(got[1], before[1]), f"{name} rank {rank}"
                ret[(rank, name)] = (got[0].cpu(), got[1].cpu())
    finally:
        dist.destroy_process_group()


def test_two_ranks_refuse_remove_items():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert set(ret.keys()) == {(r, name) for r in range(world) for name in ("brute", "naive")}
    for name in ("brute", "naive"):
        a, b = ret[(0, name)], ret[(1, name)]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name            # identical on every rank
