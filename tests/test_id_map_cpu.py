"""CPU: the host side of the item id -> position map (rails_id_map_*) -- size helpers, argument validation before any
launch, the documented hash as a bijection, the kernels' scratch use, and the host rules of the by-id calls (topk_modules.upsert_plan and
removal_plan) against a Python-dict model of the map."""
import os
import re
import subprocess

import pytest
import torch

from rails_amd import _lib
from rails_amd.topk_modules import removal_plan, upsert_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
M64 = (1 << 64) - 1
C1, C2, GAMMA = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0x9E3779B97F4A7C15
NAMES = ("rails_id_map_slots", "rails_id_map_bytes", "rails_id_map_clear", "rails_id_map_insert", "rails_id_map_erase", "rails_id_map_lookup")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def mix(x):
    z = (x + GAMMA) & M64
    z = ((z ^ (z >> 30)) * C1) & M64
    z = ((z ^ (z >> 27)) * C2) & M64
    return z ^ (z >> 31)


def unmix(h):
    z = h ^ (h >> 31) ^ (h >> 62)
    z = (z * pow(C2, -1, 1 << 64)) & M64
    z = z ^ (z >> 27) ^ (z >> 54)
    z = (z * pow(C1, -1, 1 << 64)) & M64
    z = z ^ (z >> 30) ^ (z >> 60)
    return (z - GAMMA) & M64


def test_entry_points_are_additions_under_abi_15(lib):
    header = open(os.path.join(ROOT, "include", "rails_amd.h")).read()
    assert re.search(r"#define RAILS_ABI_VERSION 15\b", header) and _lib.RAILS_ABI_VERSION == 15 and lib.rails_abi_version() == 15
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    source = open(os.path.join(ROOT, "rails_amd", "csrc", "id_map.hip")).read()
    for text in (header, source):      # the formula the tests restate is the documented one
        assert all(f"0x{c:016X}" in text for c in (C1, C2, GAMMA)) and ">> 30" in text and ">> 27" in text and ">> 31" in text


def test_size_helpers(lib):
    want = {0: 4, 1: 4, 1_024: 4_096, 1_025: 8_192}
    for n, slots in want.items():
        assert lib.rails_id_map_slots(n) == slots and slots >= 4 * max(n, 1) and slots // 2 < 4 * max(n, 1)
        assert lib.rails_id_map_bytes(slots) == 12 * slots          # int64 keys, then int32 values
    assert lib.rails_id_map_slots((1 << 31) - 1) == 1 << 33
    assert lib.rails_id_map_bytes(0) == 0 and lib.rails_id_map_bytes(12) == 0 and lib.rails_id_map_bytes(-8) == 0


def test_validation_before_any_launch(lib):
    """No device is needed: every refused call returns before it would launch.  (1 stands for a non-NULL pointer; nothing dereferences it.)"""
    bad = _lib.RAILS_EINVAL
    assert lib.rails_id_map_slots(1 << 31) == bad and "2^31" in _lib.last_error()
    assert lib.rails_id_map_slots(-1) == bad
    # a null pointer
    assert lib.rails_id_map_clear(None, 4096, None) == bad and "NULL" in _lib.last_error()
    for args in ((None, 4096, 1, None, 0, 5, 1, None), (1, 4096, None, None, 0, 5, 1, None), (1, 4096, 1, None, 0, 5, None, None)):
        assert lib.rails_id_map_insert(*args) == bad and "NULL" in _lib.last_error(), args
    for args in ((None, 4096, 1, 5, 1, None), (1, 4096, None, 5, 1, None), (1, 4096, 1, 5, None, None)):
        assert lib.rails_id_map_erase(*args) == bad and "NULL" in _lib.last_error(), args
        assert lib.rails_id_map_lookup(*args) == bad and "NULL" in _lib.last_error(), args
    # slots not a power of two
    for slots in (0, -4096, 4095, 3 << 10, 1 << 34):
        assert lib.rails_id_map_clear(1, slots, None) == bad and "power of two" in _lib.last_error(), slots
        assert lib.rails_id_map_insert(1, slots, 1, None, 0, 5, 1, None) == bad
        assert lib.rails_id_map_erase(1, slots, 1, 5, 1, None) == bad
        assert lib.rails_id_map_lookup(1, slots, 1, 5, 1, None) == bad
    # negative m
    assert lib.rails_id_map_insert(1, 4096, 1, None, 0, -1, 1, None) == bad
    assert lib.rails_id_map_erase(1, 4096, 1, -1, 1, None) == bad
    assert lib.rails_id_map_lookup(1, 4096, 1, -1, 1, None) == bad
    # positions that do not fit the table's int32 values
    assert lib.rails_id_map_insert(1, 4096, 1, None, (1 << 31) - 2, 3, 1, None) == bad and "2^31" in _lib.last_error()
    assert lib.rails_id_map_insert(1, 4096, 1, None, -1, 3, 1, None) == bad
    assert lib.rails_id_map_lookup(1, 4096, 1, (1 << 31) + 1, 1, None) == bad
    # m = 0: nothing to do, whatever the pointers
    assert lib.rails_id_map_insert(None, 4096, None, None, 0, 0, None, None) == _lib.RAILS_OK
    assert lib.rails_id_map_erase(None, 4096, None, 0, None, None) == _lib.RAILS_OK
    assert lib.rails_id_map_lookup(None, 4096, None, 0, None, None) == _lib.RAILS_OK


def test_mix_is_the_documented_bijection():
    g = torch.Generator().manual_seed(1)
    hi, lo = torch.randint(0, 1 << 32, (1000,), generator=g).tolist(), torch.randint(0, 1 << 32, (1000,), generator=g).tolist()
    values = [0, 1, M64, 1 << 63, (1 << 63) + 1, (1 << 63) + 2, (1 << 63) - 1] + [(h << 32) | l for h, l in zip(hi, lo)][:993]
    assert len(values) == 1000
    for x in values:
        assert unmix(mix(x)) == x and mix(unmix(x)) == x
    assert len({mix(x) for x in values}) == len(set(values))
    # the splitmix64 step of the hashed item tables (oracle.mol_oracle._splitmix64), on the same words
    import numpy as np
    from oracle.mol_oracle import _splitmix64
    assert _splitmix64(np.array(values, dtype=np.uint64)).tolist() == [mix(x) for x in values]


def test_id_map_kernels_use_no_scratch():
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("LLVM tools of the ROCm image not found")
    if not os.path.exists(os.path.join(ROOT, "rails_amd", "csrc", "id_map.o")):
        pytest.skip("objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "id_map"], capture_output=True, text=True, timeout=600).stdout
    rows = re.findall(r"scratch\s+(\d+) lds\s+(\d+)\s+mol::(id_map_\w+_kernel)", out)
    assert sorted(r[2] for r in rows) == ["id_map_clear_kernel", "id_map_erase_kernel", "id_map_insert_kernel", "id_map_lookup_kernel"], out
    assert all(r[0] == "0" and r[1] == "0" for r in rows), out


def test_host_rules_of_the_by_id_calls_against_a_dict_model():
    """50 random chains of upserts and removals by id.  The corpus is a Python list of ids in position order; the map is a dict kept in step the way
    the modules keep theirs (remove: the removed and the moving ids erased, the movers inserted at their holes; append: inserted).  upsert_plan
    must say which ids update where and which append in what order, and after every step the dict must be the list's inverse."""
    g = torch.Generator().manual_seed(2)
    draw = lambda hi: int(torch.randint(0, hi, (1,), generator=g))      # noqa: E731
    for chain in range(50):
        corpus = [3 * j + 1 for j in range(draw(60) + 2)]
        where = {v: p for p, v in enumerate(corpus)}
        next_new = -1
        for step in range(12):
            n = len(corpus)
            if draw(2) == 0:
                m = draw(10) + 1
                given = []
                for _ in range(m):
                    if draw(2) == 0:
                        given.append(next_new)
                        next_new -= 1
                    else:
                        given.append(corpus[draw(n)])
                given = list(dict.fromkeys(given))                    # (an id given twice is refused before the plan is asked)
                found = torch.tensor([where.get(v, -1) for v in given], dtype=torch.int64)
                upd, pos, app = upsert_plan(found)
                assert [given[j] for j in upd.tolist()] == [v for v in given if v in where], (chain, step)
                assert pos.tolist() == [where[v] for v in given if v in where]
                assert [given[j] for j in app.tolist()] == [v for v in given if v not in where], "appended in the order given"
                for j in app.tolist():
                    where[given[j]] = len(corpus)
                    corpus.append(given[j])
            else:
                m = draw(min(n - 1, 8) + 1)
                gone = [corpus[p] for p in torch.randperm(n, generator=g)[:m].tolist()]
                positions = torch.tensor([where[v] for v in gone], dtype=torch.int64)
                holes, movers = removal_plan(positions, n)
                moving = [corpus[p] for p in movers.tolist()]
                for v in gone + moving:
                    del where[v]
                for v, h in zip(moving, holes.tolist()):
                    where[v] = h
                    corpus[h] = v
                del corpus[n - m:]
                assert not set(gone) & set(corpus)
            assert where == {v: p for p, v in enumerate(corpus)}, (chain, step)
