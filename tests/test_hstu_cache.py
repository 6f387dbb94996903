"""CPU: the HSTU encoder's cached incremental decoding.  The float64 restatement of tests/_hstu_cache_ref.py reproduces the fixtures the
reference wrote (tools/gen_golden_hstu_cache.py); the bars tests/test_hstu_cache_gpu.py holds the kernel to reject the mistakes a
decode kernel could plausibly make; rails_hstu_decode[_supported] validate their arguments without a device; the module refuses CPU
tensors and training mode."""
import ctypes as C
import os

import pytest
import torch

from tests import _hstu_cache_ref as R

# (bug, the scenarios where it shows): each must put some checked quantity outside its bar
BUG_CASES = [
    ("ts_p", ("tail", "tail2", "interior", "ts")),       # the query's timestamp ts[p] in place of ts[p + 1]
    ("drop_self", R.TAGS),                               # key j = p left out
    ("stale_k", R.TAGS),                                 # key p read from the cache before this row's k is written
    ("write_p", R.TAGS),                                 # v / outputs written at row p instead of the jagged row
    ("return_p", ("interior", "ts")),                    # the delta row returned instead of lengths - 1
    ("no_outputs", R.TAGS),                              # the layer output never written into the cache
]


@pytest.fixture(scope="module")
def replay():
    return {n: R.expected(n) for n in R.NAMES}


@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_reproduces_the_reference_fixtures(replay, name):
    z = R.load(name)[-1]
    e = replay[name]
    for tag in R.TAGS:
        for q in ("prefill_current", "current") + R.ROWS:
            err = float((torch.from_numpy(z[f"{tag}/{q}"]).double() - e[tag][q]).abs().max())
            assert err < 2e-5, (tag, q, err)
    if "sample/rows" in z.files:                        # the prefill's states at sampled rows
        cfg, w, lengths, ids, ts, _ = R.load(name)
        _, st = R.prefill(cfg, {k: v.double() for k, v in w.items()}, lengths, ids, ts)
        rows = torch.from_numpy(z["sample/rows"])
        for l, (v, q, k, o) in enumerate(st):
            for key, t in (("v", v[rows]), ("outputs", o[rows]), ("q", q[0]), ("k", k[0])):
                assert float((torch.from_numpy(z[f"sample/l{l}/{key}"]).double() - t).abs().max()) < 2e-5, (l, key)
    if "full/l0/v" in z.files:
        for l, st in enumerate(e["interior"]["states"]):
            for q, t in zip(R.ROWS, st):
                assert float((torch.from_numpy(z[f"full/l{l}/{q}"]).double() - t).abs().max()) < 2e-5, (l, q)


@pytest.mark.parametrize("name", R.NAMES)
def test_interior_delta_returns_the_prefill_embedding(replay, name):
    """The reference's quirk the module keeps: a delta before lengths - 1 leaves the returned row stale."""
    z = R.load(name)[-1]
    for tag in ("interior", "ts"):
        pos, lengths = torch.from_numpy(z[f"{tag}/positions"]), torch.from_numpy(z["in/past_lengths"])
        assert bool((pos < lengths - 1).any())
        stale = pos < lengths - 1
        assert torch.equal(torch.from_numpy(z[f"{tag}/current"])[stale], torch.from_numpy(z[f"{tag}/prefill_current"])[stale])


@pytest.mark.parametrize("bug,tags", BUG_CASES, ids=[b for b, _ in BUG_CASES])
@pytest.mark.parametrize("name", R.NAMES)
def test_bars_reject_plausible_decode_bugs(replay, name, bug, tags):
    good = replay[name]
    bars = R.bars(name, good)
    bad = R.expected(name, bug=bug)
    caught = [(tag, q) for tag in tags for q in ("current",) + R.ROWS
              if float((bad[tag][q] - good[tag][q]).abs().max()) > bars[tag][q]]
    assert caught, (name, bug)


def test_decode_entry_points_validate_without_a_device():
    from rails_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    # the three shipped geometries at their real sizes, and the per-layer encoder's head limits at D = 1024
    for N, D, H, dh, nb in ((211, 50, 2, 25, 128), (211, 256, 8, 32, 128), (61, 64, 8, 8, 128), (4096, 1024, 16, 32, 255), (1, 1, 1, 1, 0)):
        assert lib.rails_hstu_decode_supported(N, D, H, dh, dh, nb) == 1, (N, D, H, dh)
    for N, D, H, dqk, dv, nb in ((211, 1025, 2, 25, 25, 128), (211, 256, 8, 33, 32, 128), (211, 256, 8, 32, 33, 128), (211, 256, 8, 32, 32, 256),
                                 (0, 256, 8, 32, 32, 128), (211, 1024, 512, 32, 32, 128)):
        assert lib.rails_hstu_decode_supported(N, D, H, dqk, dv, nb) == 0, (N, D, H, dqk, dv, nb)

    def call(batch=2, n_blocks=1, N=16, rows=4, D=64, H=2, dqk=8, dv=8, nb=128, act=1, mode=0, ts=None, thr=None, ptr=None):
        return lib.rails_hstu_decode(ptr, ptr, ptr, ptr, ts, thr, ptr, ptr, n_blocks, batch, N, rows, D, H, dqk, dv, nb, act, mode,
                                     C.c_float(1e-6), ptr, None)

    assert call(batch=0) == _lib.RAILS_OK                                   # nothing to do, nothing launched
    assert call() == _lib.RAILS_EINVAL and "NULL" in _lib.last_error()
    for kw in (dict(batch=-1), dict(n_blocks=0), dict(N=0), dict(D=0), dict(H=0), dict(dqk=0), dict(dv=0), dict(rows=1), dict(act=2),
               dict(mode=2), dict(ts=C.c_void_p(16), thr=None)):
        assert call(**kw) == _lib.RAILS_EINVAL, kw
    for kw in (dict(D=1025), dict(dqk=33), dict(dv=40), dict(nb=256)):
        assert call(batch=0, **kw) == _lib.RAILS_ENOTSUP and "not supported" in _lib.last_error(), kw


def test_decode_refuses_cpu_tensors_and_training():
    from tests.test_hstu_kernels_gpu import module, sequences

    m, cfg, w = module(16, 64, 2, 2, 8, 8, "layer_norm")
    lengths, ids, ts = sequences(2, 16, seed=1)
    emb = m.get_item_embeddings(ids)
    pos = lengths - 1
    delta = (torch.cumsum(lengths, 0) - lengths + pos, pos)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.encode(lengths, ids, emb, {"timestamps": ts}, delta_x_offsets=delta, cache=[None, None])
    with pytest.raises(RuntimeError, match="GPU only"):
        m.encode(lengths, ids, emb, {"timestamps": ts}, return_cache_states=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.generate_user_embeddings(lengths, ids, emb, {"timestamps": ts}, delta_x_offsets=delta, cache=[None, None])
    m.train()
    with pytest.raises(NotImplementedError, match="eval-only"):
        m.encode(lengths, ids, emb, {"timestamps": ts}, delta_x_offsets=delta, cache=[None, None])
    with pytest.raises(NotImplementedError, match="eval-only"):
        m.generate_user_embeddings(lengths, ids, emb, {"timestamps": ts}, return_cache_states=True)
