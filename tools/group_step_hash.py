"""Same bytes on the group path?  One lumen_group step of the benchmark's job on WORLD contexts of device 0 (the transport
LUMEN_TRANSPORT_AUTO picks: copies), every output hashed into OUT.json -- the Merkle root, the queried columns, all gathered
digests, every rank's MatR and MatZ, three encoded and three level-1 columns per rank.  bench.py --dump-outputs is one GPU
only; this is its counterpart for lm_group.hip.  Run it from the root of each of two trees and compare the files (every
key but "tree" must be equal):

    python tools/group_step_hash.py 4096x2048 4 OUT.json"""
import hashlib, json, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import bench  # noqa: F401  (puts the tree on sys.path the way the benchmark does)
from bench_lib.job import Job
from lumenos_amd.hip import Group
import lumenos_amd
cfg, world, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
job = Job(cfg, 0, world, 0, 0, False, [0] * world)
job.group = Group(job.ctxs, transport="auto")
res = {"tree": os.path.dirname(os.path.abspath(lumenos_amd.__file__)), "config": cfg, "world": world, "transport": job.group.transport,
       "note": job.group.transport_note}
def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
job.step_group()  # once to warm the pools: the kept step below recycles blocks
enc, lvl1, mat_r, mat_z, q, root = job.step_group(keep=True)
res["root"] = root.hex()
res["queried_cols"] = h(q.download())
for name, sets in (("mat_r", mat_r), ("mat_z", mat_z)):
    res[name] = [h(s.download()) for s in sets]
for name, sets in (("enc", enc), ("lvl1", lvl1)):
    res[name] = [[h(s.download(k, 1)) for k in sorted({0, s.count // 3, s.count - 1})] for s in sets]
res["digests"] = h(job.group.digests(job.S))
res["stats_calls"] = {n: job.group.stats(n)[2] for n in ("all_to_all_1", "all_to_all_2", "all_gather", "gather_to_root")}
json.dump(res, open(out, "w"), indent=1, sort_keys=True)
print(json.dumps({k: res[k] for k in ("tree", "transport", "root", "queried_cols", "stats_calls")}))
job.close()
