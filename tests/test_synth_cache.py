"""CPU checks of the stored copies of bench.py's inputs (kmeranno.synth_cache) and of
bench.dump_outputs: a copy gives back exactly what the generator makes, is found only under the
arguments it was stored with, and an output above the dump's byte budget is cut to the same
sample every time."""
import os

import numpy as np

ARGS = (3_000, 50, 7, 8, 40, 99)  # table rows, functions, seed, k, proteins, query seed


def test_stored_copy_equals_generator(tmp_path, monkeypatch):
    from kmeranno import synth, synth_cache
    monkeypatch.setenv("KMA_SYNTH_CACHE", str(tmp_path))
    assert synth_cache.load_table(*ARGS[:4]) is None and synth_cache.load_queries(*ARGS) is None
    assert synth_cache.store(*ARGS) is True
    assert synth_cache.store(*ARGS) is False  # both copies are there: nothing generated
    sig = synth.make_table(*ARGS[:4])
    got = synth_cache.load_table(*ARGS[:4])
    assert got.n_fid == sig.n_fid and len(got.protos) == len(sig.protos)
    assert all((a == b).all() and a.dtype == b.dtype for a, b in zip(got.protos, sig.protos))
    for a, b in ((got.keys, sig.keys), (got.fids, sig.fids)):
        assert a.dtype == b.dtype and (a == b).all()
    for a, b in zip(synth_cache.load_queries(*ARGS), synth.make_queries(sig, *ARGS[4:])):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    # queries made from the stored prototypes are the generator's too
    for a, b in zip(synth.make_queries(got, 25, 5), synth.make_queries(sig, 25, 5)):
        assert (a == b).all()
    # other arguments: no copy
    assert synth_cache.load_table(3_001, *ARGS[1:4]) is None
    assert synth_cache.load_queries(*ARGS[:5], 100) is None
    assert not [f for f in os.listdir(tmp_path) if "." in f]  # no half-written copy left


def test_dump_outputs_budget_and_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * (8 * 1000 + 128))  # 2 arrays of 1000 rows
    big = np.arange(5000, dtype=np.int32) * 3
    small = np.arange(10, dtype=np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, {"big": big, "small": small})
    a, b = (np.load(tmp_path / d / "big.npy") for d in ("a", "b"))
    assert a.dtype == np.float64 and len(a) == 1000 and (a == b).all()
    assert (np.diff(a) > 0).all() and np.isin(a, big).all()
    assert (np.load(tmp_path / "a" / "small.npy") == small).all()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) \
        <= bench.DUMP_BUDGET
    bench.dump_outputs(str(tmp_path / "a"), 1, {"small": small})
    assert os.path.exists(tmp_path / "a" / "small.rank1.npy")
