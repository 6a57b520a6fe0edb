"""On-disk copies of the seeded synth workloads bench.py times.

The generators of synth.py are deterministic but slow at the north-star size (c5: 10^8 table
rows and 1M proteins take most of a minute of numpy on one core). store() runs them once and
keeps their arrays as .npy files; load() returns the very same arrays in about a second. The
files are a cache and nothing more: a missing, stale or unreadable one makes load() return None
and the caller generates. A copy is stale when synth.py, the CDS length file, numpy's version or
the arguments differ from what it was written under (all of them are in its directory's name).

The copies live under kmers.anno_amd/build/synth_cache (with the other build products), or
under $KMA_SYNTH_CACHE. store() is called by the build (__graft_entry__.build), never by a
benchmark run or a test.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import tempfile

import numpy as np

from . import synth

_HERE = os.path.dirname(os.path.abspath(__file__))


def cache_root() -> str:
    return os.environ.get("KMA_SYNTH_CACHE") or os.path.normpath(
        os.path.join(_HERE, "..", "..", "build", "synth_cache"))


def _generator_digest() -> str:
    h = hashlib.sha256(np.__version__.encode())
    for path in (synth.__file__, synth._LEN_FILE):
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _dir(kind: str, *args) -> str:
    return os.path.join(cache_root(), f"{kind}_{'_'.join(map(str, args))}_{_generator_digest()}")


def _table_dir(table_size, n_fid, seed, k):
    return _dir("table", table_size, n_fid, seed, k)


def _queries_dir(table_size, n_fid, seed, k, n_seq, query_seed):
    return _dir("queries", table_size, n_fid, seed, k, n_seq, query_seed)


def _write(path: str, arrays: dict) -> None:
    """All of a copy's files appear at once (a rename), so a reader never sees half of one."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = tempfile.mkdtemp(prefix=os.path.basename(path) + ".", dir=os.path.dirname(path))
    try:
        for name, a in arrays.items():
            np.save(os.path.join(tmp, name + ".npy"), a)
        os.rename(tmp, path)
    except OSError:
        shutil.rmtree(tmp, ignore_errors=True)
        if not os.path.isdir(path):  # (another process may have stored the same copy first)
            raise


def _read(path: str, names) -> dict | None:
    try:
        return {n: np.load(os.path.join(path, n + ".npy")) for n in names}
    except (OSError, ValueError):
        return None


def load_table(table_size: int, n_fid: int, seed: int, k: int = 8) -> synth.SignatureSet | None:
    """synth.make_table(table_size, n_fid, seed, k) from its stored copy, or None."""
    d = _read(_table_dir(table_size, n_fid, seed, k), ("keys", "fids", "protos", "proto_off"))
    if d is None:
        return None
    off = d["proto_off"]
    protos = [d["protos"][int(off[i]):int(off[i + 1])] for i in range(n_fid)]
    return synth.SignatureSet(protos, d["keys"], d["fids"], n_fid)


def load_queries(table_size: int, n_fid: int, seed: int, k: int, n_seq: int, query_seed: int):
    """synth.make_queries(make_table(...), n_seq, query_seed) from its stored copy, or None."""
    d = _read(_queries_dir(table_size, n_fid, seed, k, n_seq, query_seed),
              ("residues", "offsets", "kinds", "true_fid"))
    if d is None:
        return None
    return d["residues"], d["offsets"], d["kinds"], d["true_fid"]


def store(table_size: int, n_fid: int, seed: int, k: int, n_seq: int, query_seed: int) -> bool:
    """Generate and keep one table and one query batch unless both copies are there already.
    Returns whether anything was generated."""
    tdir = _table_dir(table_size, n_fid, seed, k)
    qdir = _queries_dir(table_size, n_fid, seed, k, n_seq, query_seed)
    have_t, have_q = os.path.isdir(tdir), os.path.isdir(qdir)
    if have_t and have_q:
        return False
    sig = synth.make_table(table_size, n_fid, seed, k, protos_only=have_t)
    if not have_t:
        proto_off = np.zeros(n_fid + 1, np.int64)
        np.cumsum([len(p) for p in sig.protos], out=proto_off[1:])
        _write(tdir, {"keys": sig.keys, "fids": sig.fids, "protos": np.concatenate(sig.protos),
                      "proto_off": proto_off})
    if not have_q:
        res, off, kinds, true_fid = synth.make_queries(sig, n_seq, query_seed)
        _write(qdir, {"residues": res, "offsets": off, "kinds": kinds, "true_fid": true_fid})
    return True
