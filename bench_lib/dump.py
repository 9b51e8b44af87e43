"""bench.py --dump-outputs DIR: what the timed path handed its caller in its last step -- MatR, MatZ, the queried
columns, the Merkle tree and its root (with --ring-switch-logn also MatR / MatZ in the small ring) -- as .npy files, so
that two builds of the project can be compared output for output on the same seeded inputs."""
import os

import numpy as np

# residues per sampled array: 2^19 (8 MB as float64 word pairs); the largest run writes about 30 MB in all
MAX_WORDS = 1 << 19
SAMPLE_CTS = 32
LIMIT_BYTES = 64 << 20


def residues_f64(a):
    """uint64 residues (moduli of up to 60 bits: more than float64's 53-bit mantissa holds) as exact float64 pairs on
    a new last axis: (low 32 bits, high 32 bits)"""
    a = np.asarray(a, dtype=np.uint64)
    return np.stack([a & np.uint64(0xFFFFFFFF), a >> np.uint64(32)], axis=-1).astype(np.float64)


def sample(count, fetch, seed):
    """A fixed, seeded sample of `count` ciphertexts: up to SAMPLE_CTS of them at seeded positions (all when there are
    no more), fetched one at a time (fetch(i) -> array [1, ...]), and when those hold more than MAX_WORDS residues,
    the same seeded positions of the last axis (the coefficients) of each."""
    rng = np.random.default_rng(seed)
    pick = np.arange(count) if count <= SAMPLE_CTS else np.sort(rng.choice(count, size=SAMPLE_CTS, replace=False))
    data = np.concatenate([fetch(int(i)) for i in pick])
    if data.size > MAX_WORDS:
        n = data.shape[-1]
        keep = max(1, MAX_WORDS * n // data.size)
        data = data[..., np.sort(rng.choice(n, size=keep, replace=False))]
    return data


def dump_outputs(out_dir, job, outs):
    """outs: what Job.step(keep=True) returned -- MatR, MatZ and the queried columns (device sets), the Merkle tree's
    nodes and its root.  Writes out_dir/<name>.npy: float64 word pairs for residues, float32 for bytes."""
    mat_r, mat_z, q, nodes, root = outs
    arrays = {}
    for k, (name, s) in enumerate((("mat_r", mat_r), ("mat_z", mat_z), ("queried_cols", q))):
        arrays[name] = residues_f64(sample(s.count, lambda i, s=s: s.download(i, 1), seed=100 + k))
    if job.ring_switch_logn:  # MatR / MatZ as they leave for the proof: page-locked host arrays the step wrote
        for k, (name, h) in enumerate((("mat_r_ring_switched", job.h_rs[0]), ("mat_z_ring_switched", job.h_rs[1]))):
            arrays[name] = residues_f64(sample(len(h), lambda i, h=h: h[i:i + 1], seed=200 + k))
    arrays["merkle_nodes"] = np.asarray(nodes, dtype=np.uint8).astype(np.float32)
    arrays["merkle_root"] = np.frombuffer(root, dtype=np.uint8).astype(np.float32)
    total = sum(a.nbytes for a in arrays.values())
    if total > LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {LIMIT_BYTES}-byte budget")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
