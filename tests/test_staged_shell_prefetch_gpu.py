"""The staged scoring shells (mol_score_shell.h: mol_score_staged_kernel, mol_score_staged1_kernel) prefetch the next item tile into
LDS by LDS-DMA while the waves work on the current one.  Where in a tile's work the prefetch is issued is a matter of speed alone: the
logits must be the bits the independent-wave shell computes from the same packs (it reads every fragment straight from memory: no LDS
tile, no DMA, no barrier), and the same bits on every call -- a tile consumed before it had landed, or overwritten while a wave still
read it, would show as a difference between two calls or against the independent-wave route.

Corpora are the smallest that take the staged routes the way the headline does: 8 rounds of tiles for the device's CU count (the
dispatcher's line for the double-buffered shell, choose_variant) plus 1, 31 and 33 items, so that the last round is ragged and the
last tile partial.  B = 32 is the headline batch (one query group per wave); B = 35 wraps the group loop (nine groups on eight
waves) and ends in a padded group.

The independent-wave route: fp32 -- rails_mol_score_indexed with every position of the index as every row's candidates; f16x3 --
per-row candidates (rails_mol_index_gather + rails_mol_score_candidates) over every position, in column chunks."""
import dataclasses
import functools

import pytest
import torch

from oracle import mol_oracle as O

SHAPES = {"8x8x32": ("amzn-books", "staged"), "8x4x64": ("ml-1m", "staged"), "8x4x128": ("ml-20m", "staged1")}
EXTRA = (1, 31, 33)
BATCHES = (32, 35)
CHUNK = 16384          # columns per gathered per-row chunk (a multiple of the 32-item tile)
LDS = 160 * 1024
WAVES = 8


def route(cfg, B, N, n_cu):
    """choose_variant (mol_score_shell.h) for a shared corpus, restated."""
    pq, px, d, h = cfg.query_dot_product_groups, cfg.item_dot_product_groups, cfg.dot_product_dimension, cfg.gating_qi_hidden_dim
    L = pq * px
    wpack, ex, gi = h * L + L * h + h + L, 32 * px * d, 32 * L
    n_groups, n_tiles = -(-B // (32 // pq)), -(-N // 32)
    staged_fits, staged1_fits = 4 * (wpack + 2 * (ex + gi)) <= LDS, 4 * (wpack + ex + 2 * gi) <= LDS
    if n_groups >= WAVES:
        if staged_fits and n_tiles >= 8 * n_cu:
            return "staged"
        if staged1_fits:
            return "staged1"
        if staged_fits:
            return "staged"
    return "direct"


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def n_cu():
    from rails_amd import _lib

    n = int(_lib.load().rails_device_compute_units())
    assert n > 0
    return n


@functools.lru_cache(maxsize=None)
def setup(shape, precision, B, N):
    """(engine, query pack, index) on cuda:0 -- one per case, shared by its tests."""
    from rails_amd import engine as E

    dev = torch.device("cuda", 0)
    cfg = O.CONFIGS[SHAPES[shape][0]]
    w = O.synthetic_weights(cfg, seed=3)
    names = {f.name for f in dataclasses.fields(E.MolShapeSpec)}
    spec = E.MolShapeSpec(**{k: v for k, v in dataclasses.asdict(cfg).items() if k in names})
    eng = E.MolEngine(spec, {k: v.to(dev) for k, v in w.items()}, precision=precision)
    uid = torch.arange(B, dtype=torch.int64, device=dev) * 37 + 1 if cfg.uid_embedding_hash_sizes else None
    pack, _, _ = eng.query_pack(O.synthetic_queries(cfg, B, seed=B).to(dev), uid)
    index = eng.build_index(E.hash_item_table(5, 0, N, cfg.item_embedding_dim, dev))
    return cfg, eng, pack, index


def staged_logits(eng, pack, B, index):
    out = torch.full((B, index.n_items), float("nan"), dtype=torch.float32, device=index.buf.device)   # a fresh buffer, no stale logits
    return eng.score_dense(pack, B, index, out=out)


def independent_wave_logits(eng, pack, B, index, precision):
    N, dev = index.n_items, index.buf.device
    if precision == "fp32":
        assert eng.score_indexed_supported(B, N)
        return eng.score_indexed(pack, B, index, torch.arange(N, device=dev).expand(B, N))
    out = torch.empty((B, N), dtype=torch.float32, device=dev)
    for c0 in range(0, N, CHUNK):
        c1 = min(N, c0 + CHUNK)
        cidx, kp = eng.gather_index(index, torch.arange(c0, c1, device=dev).expand(B, c1 - c0))
        out[:, c0:c1] = eng.score_candidates(pack, B, cidx, kp)[:, : c1 - c0]
    return out


CASES = [(s, p, b, e) for s in SHAPES for p in ("fp32", "f16x3") for b in BATCHES for e in EXTRA]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,precision,B,extra", CASES, ids=lambda v: str(v))
def test_staged_logits_are_the_bits_of_the_independent_wave_shell(dev, n_cu, shape, precision, B, extra):
    N = 32 * 8 * n_cu + extra
    cfg, eng, pack, index = setup(shape, precision, B, N)
    assert route(cfg, B, N, n_cu) == SHAPES[shape][1]
    got = staged_logits(eng, pack, B, index)
    ref = independent_wave_logits(eng, pack, B, index, precision)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()), "a column the staged shell did not write"
    diff = got != ref
    assert not bool(diff.any()), (f"{int(diff.sum())} of {diff.numel()} logits differ; first at {tuple(int(t) for t in diff.nonzero()[0])}, "
                                  f"max |d| {float((got - ref).abs().max()):.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,precision,B,extra", CASES, ids=lambda v: str(v))
def test_staged_logits_are_the_same_bits_on_every_call(dev, n_cu, shape, precision, B, extra):
    N = 32 * 8 * n_cu + extra
    cfg, eng, pack, index = setup(shape, precision, B, N)
    assert route(cfg, B, N, n_cu) == SHAPES[shape][1]
    outs = [staged_logits(eng, pack, B, index) for _ in range(10)]
    torch.cuda.synchronize()
    for i, o in enumerate(outs[1:], 1):
        diff = o != outs[0]
        assert not bool(diff.any()), f"call {i}: {int(diff.sum())} logits differ from call 0; first at {tuple(int(t) for t in diff.nonzero()[0])}"
