"""Multi-process distributed tests on the CPU TCP comm engine.

Exercises the deterministic SPMD dataflow protocol (sends/recvs, channel
sequencing, flush_all, barrier) with world_size 2 and 4 on one host —
the reference tests multi-node the same way (multiple ranks on one host,
SURVEY.md §4).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "_dist_worker.py")

from conftest import port_base

# every test below takes its ports from this one window: 126 in all
_next_port = [port_base(span=128)]


def communicate_all(procs, timeout=180):
    """Wait for every worker and return their outputs. A worker that dies
    leaves its peers blocked on it, so on a timeout all are ended and the
    failure shows every worker's output, the dead one's error included."""
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=timeout)[0].decode())
    except subprocess.TimeoutExpired:
        for pr in procs:
            pr.kill()
        outs = [pr.communicate()[0].decode() for pr in procs]
        report = "\n".join(f"--- rank {r} (exit {pr.returncode}):\n{o}"
                           for r, (pr, o) in enumerate(zip(procs, outs)))
        pytest.fail(f"workers still running after {timeout} s:\n{report}")
    return outs


def run_world(world, tmpdir, p, q, n=256, nb=64):
    port = _next_port[0]
    _next_port[0] += world + 2
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world),
                   PARSEC_TEST_PORT=str(port), PARSEC_TEST_OUT=str(tmpdir),
                   GRID_P=str(p), GRID_Q=str(q), MAT_N=str(n), MAT_NB=str(nb))
        procs.append(subprocess.Popen([sys.executable, WORKER], env=env,
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    outs = communicate_all(procs)
    for pr, out in zip(procs, outs):
        assert pr.returncode == 0, f"worker failed:\n{out}"
    # assemble
    pre = np.zeros((n, n))
    post = np.zeros((n, n))
    for r in range(world):
        z = np.load(os.path.join(tmpdir, f"rank{r}.npz"))
        for key in z.files:
            kind, tm, tn = key.split("_")[0], *key.split("_")[1:]
            tm, tn = int(tm), int(tn)
            v = z[key]
            dst = pre if kind == "pre" else post
            dst[tm * nb:tm * nb + v.shape[0], tn * nb:tn * nb + v.shape[1]] = v
    return pre, post


@pytest.mark.parametrize("world,p,q", [(2, 2, 1), (2, 1, 2), (4, 2, 2), (8, 2, 4)])
def test_distributed_cholesky(world, p, q, tmp_path):
    pre, post = run_world(world, tmp_path, p, q)
    M = np.tril(pre) + np.tril(pre, -1).T
    L0 = np.linalg.cholesky(M)
    err = np.abs(np.tril(post) - L0).max()
    assert err < 1e-10, f"world={world} p={p} q={q}: max err {err}"


def test_distributed_qr(tmp_path):
    """World-2 tile QR over the TCP engine: checks workspace-collection
    transfers (V2/T1 tiles) and flush; verified via R^T R == A^T A."""
    world, p, q, n, nb = 2, 2, 1, 256, 64
    port = _next_port[0]
    _next_port[0] += world + 2
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world),
                   PARSEC_TEST_PORT=str(port), PARSEC_TEST_OUT=str(tmp_path),
                   GRID_P=str(p), GRID_Q=str(q), MAT_N=str(n), MAT_NB=str(nb),
                   PARSEC_TEST_APP="qr")
        procs.append(subprocess.Popen([sys.executable, WORKER], env=env,
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for pr, out in zip(procs, communicate_all(procs)):
        assert pr.returncode == 0, f"worker failed:\n{out}"
    pre = np.zeros((n, n))
    post = np.zeros((n, n))
    for r in range(world):
        z = np.load(os.path.join(tmp_path, f"rank{r}.npz"))
        for key in z.files:
            kind, tm, tn = key.split("_")[0], *key.split("_")[1:]
            tm, tn = int(tm), int(tn)
            v = z[key]
            dst = pre if kind == "pre" else post
            dst[tm * nb:tm * nb + v.shape[0], tn * nb:tn * nb + v.shape[1]] = v
    R = np.triu(post)
    err = np.abs(R.T @ R - pre.T @ pre).max() / np.abs(pre.T @ pre).max()
    assert err < 1e-12, f"distributed QR rel err {err}"


FUZZ_CODE = r"""
import os, sys
sys.path.insert(0, os.environ["PARSEC_REPO"])
import random
import numpy as np
import parsec_amd as pm

rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=world, comm="tcp", gpu=-2)
rng = random.Random(int(os.environ["SEED"]))  # identical on all ranks
NT, nb = int(os.environ.get("FUZZ_NT", "10")), 16
A = pm.TiledMatrix(ctx, NT * nb, nb, nb, nb, world, 1)
if rng.random() < 0.3:
    # ~1/3 of seeds run on a random rank table (two_dim_tabular analog):
    # owner placement drives every SPMD channel decision, so shuffle it
    table = [rng.randrange(world) for _ in range(NT)]
    A.set_rank_table(table)
tp = pm.Dtd(ctx, "fuzz")
oracle = []
for i in range(NT):
    # non-symmetric so transposed (reshape-promise) reads are observable
    v = np.arange(nb * nb, dtype=np.float64).reshape(nb, nb) * 1e-3 + i + 1
    oracle.append(v.copy())
    if A.is_local(i, 0):
        A.tile_numpy_set(i, 0, v)
ctx.barrier()

for step in range(int(os.environ.get("OPS", "150"))):
    target = rng.randrange(NT)
    nsrc = rng.randrange(0, 3)
    srcs = rng.sample([i for i in range(NT) if i != target], nsrc)
    exec_rank = rng.randrange(world)
    coeffs = [round(rng.uniform(-1, 1), 3) for _ in range(nsrc + 1)]
    # ~1/4 of reads consume the TRANSPOSED copy (reshape promise)
    trans = [rng.random() < 0.25 for _ in srcs]
    write_only = nsrc == 0 and rng.random() < 0.3
    # oracle replay (pure numpy, every rank computes the same)
    if write_only:
        oracle[target] = np.full((nb, nb), coeffs[0])
    else:
        acc = coeffs[0] * oracle[target]
        for c, s, tr in zip(coeffs[1:], srcs, trans):
            acc = acc + c * (oracle[s].T if tr else oracle[s])
        oracle[target] = acc
    # task body (only runs on exec_rank)
    def body(tbuf, *sbufs, coeffs=coeffs, write_only=write_only):
        t = np.frombuffer(tbuf, dtype=np.float64)
        if write_only:
            t[:] = coeffs[0]
            return
        acc = coeffs[0] * t
        for c, sb in zip(coeffs[1:], sbufs):
            acc = acc + c * np.frombuffer(sb, dtype=np.float64)
        t[:] = acc
    flows = [(A.tile(target, 0),
              pm.ACCESS_OUT if write_only else pm.ACCESS_INOUT)]
    flows += [(A.tile(s, 0), pm.ACCESS_IN, pm.RESHAPE_TRANSPOSE) if tr
              else (A.tile(s, 0), pm.ACCESS_IN)
              for s, tr in zip(srcs, trans)]
    tp.insert_py(body, flows=flows, rank=exec_rank, with_data=True)

tp.wait()
tp.flush_all(A)
tp.wait()
ctx.barrier()
bad = 0
for i in range(NT):
    if A.is_local(i, 0):
        got = A.tile_numpy(i, 0)
        if not np.allclose(got, oracle[i], atol=1e-9):
            print(f"rank {rank}: tile {i} diverged "
                  f"(max err {np.abs(got - oracle[i]).max()})")
            bad += 1
assert bad == 0
print("FUZZ_OK", rank)
ctx.barrier()
del A, ctx
"""


@pytest.mark.parametrize("world,seed,tree", [
    (2, 101, "unicast"), (2, 202, "unicast"), (4, 303, "unicast"),
    (8, 404, "unicast"), (4, 505, "binomial"), (8, 606, "binomial")])
def test_distributed_fuzz_vs_oracle(world, seed, tree, tmp_path):
    """Random DAGs (random tiles/modes/executing ranks) through the full
    SPMD protocol must match a sequential numpy oracle — with both the
    unicast and the binomial-tree fan-out (renaming + flow control live
    underneath in all cases)."""
    port = _next_port[0]
    _next_port[0] += world + 2
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world), PORT=str(port),
                   SEED=str(seed), PARSEC_REPO=os.path.dirname(HERE),
                   PARSEC_MCA_bcast_tree=tree)
        procs.append(subprocess.Popen([sys.executable, "-c", FUZZ_CODE],
                                      env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for pr in procs:
        out, _ = pr.communicate(timeout=180)
        assert pr.returncode == 0 and b"FUZZ_OK" in out, out.decode()


def test_distributed_lu(tmp_path):
    """World-4 tile LU nopiv over the TCP engine: L*U == A."""
    world, p, q, n, nb = 4, 2, 2, 256, 64
    port = _next_port[0]
    _next_port[0] += world + 2
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world),
                   PARSEC_TEST_PORT=str(port), PARSEC_TEST_OUT=str(tmp_path),
                   GRID_P=str(p), GRID_Q=str(q), MAT_N=str(n), MAT_NB=str(nb),
                   PARSEC_TEST_APP="lu")
        procs.append(subprocess.Popen([sys.executable, WORKER], env=env,
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for pr, out in zip(procs, communicate_all(procs)):
        assert pr.returncode == 0, f"worker failed:\n{out}"
    pre = np.zeros((n, n))
    post = np.zeros((n, n))
    for r in range(world):
        z = np.load(os.path.join(tmp_path, f"rank{r}.npz"))
        for key in z.files:
            kind, tm, tn = key.split("_")[0], *key.split("_")[1:]
            tm, tn = int(tm), int(tn)
            v = z[key]
            dst = pre if kind == "pre" else post
            dst[tm * nb:tm * nb + v.shape[0], tn * nb:tn * nb + v.shape[1]] = v
    L = np.tril(post, -1) + np.eye(n)
    U = np.triu(post)
    err = np.abs(L @ U - pre).max() / np.abs(pre).max()
    assert err < 1e-11, f"distributed LU rel err {err}"


def test_pingpong_benchmark(tmp_path):
    """The ping-pong harness (rtt/bandwidth.jdf analog) runs and reports."""
    port = _next_port[0]
    _next_port[0] += 4
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE="2",
                   PARSEC_MCA_comm_base_port=str(port),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port + 2))
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(os.path.dirname(HERE),
                                          "benchmarks", "bench_pingpong.py"),
             "--hops", "40", "--sizes", "4096"],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for pr in procs:
        # generous: the gloo rendezvous + 2-proc startup can crawl when the
        # host is loaded (observed once under a concurrent full-suite soak)
        out, _ = pr.communicate(timeout=300)
        outs.append(out.decode())
        assert pr.returncode == 0, out.decode()
    assert any("rtt_us" in o for o in outs), outs


def test_rccl_fallback_to_tcp(tmp_path):
    """init_distributed falls back to the TCP engine when RCCL cannot
    come up (here: no GPU) — agreed across ranks via gloo."""
    code = r"""
import os, sys
sys.path.insert(0, os.environ["PARSEC_REPO"])
import parsec_amd as pm
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.init_distributed(nworkers=2, comm="rccl", gpu=-2)
assert ctx.world == 2
A = pm.TiledMatrix(ctx, 256, 256, 64, 64, 2, 1)
tp = pm.Dtd(ctx)
pm.insert_spd_fill(tp, A, 3)
pm.insert_potrf(tp, A)
tp.wait()
ctx.barrier()
print("FALLBACK_OK", ctx.rank)
del A, ctx
"""
    port = _next_port[0]
    _next_port[0] += 4
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE="2", PORT=str(port),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port + 2),
                   PARSEC_REPO=os.path.dirname(HERE))
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env,
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for pr in procs:
        out, _ = pr.communicate(timeout=180)
        assert pr.returncode == 0 and b"FALLBACK_OK" in out, out.decode()


def test_all_to_all_redistribute(tmp_path):
    """a2a.jdf analog: (4,1)->(1,4) grid transpose is a full all-to-all;
    every rank exchanges tiles with every other rank."""
    world = 4
    code = f"""
import os, sys
sys.path.insert(0, {os.path.dirname(HERE)!r})
import numpy as np
import parsec_amd as pm
rank = int(os.environ["RANK"])
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=4, comm="tcp", gpu=-2)
nt, nb = 8, 16
S = pm.TiledMatrix(ctx, nt * nb, nt * nb, nb, nb, 4, 1)
D = pm.TiledMatrix(ctx, nt * nb, nt * nb, nb, nb, 1, 4)
tp = pm.Dtd(ctx, "a2a")
pm.insert_full_fill(tp, S, 13)
pm.insert_redistribute(tp, S, D)
tp.wait()
ctx.barrier()
ok = 0
for i in range(nt):
    for j in range(nt):
        if D.is_local(i, j):
            v = D.tile_numpy(i, j)
            assert np.isfinite(v).all() and abs(v).max() > 0
            ok += 1
c = ctx.counters()
assert c["comm_msgs"] > 0  # every rank both sent and received
print("A2A_OK", rank, ok)
ctx.barrier()
del S, D, ctx
"""
    port = _next_port[0]
    _next_port[0] += world + 2
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world), PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env,
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for pr in procs:
        o, _ = pr.communicate(timeout=180)
        assert pr.returncode == 0 and b"A2A_OK" in o, o.decode()


def test_peer_death_detected(tmp_path):
    """A rank dying mid-run makes the survivor fail loudly (connection
    lost), not hang — the failure-detection behavior the runtime owns."""
    code_survivor = f"""
import os, sys
sys.path.insert(0, {os.path.dirname(HERE)!r})
import parsec_amd as pm
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=0, world=2, comm="tcp", gpu=-2)
A = pm.TiledMatrix(ctx, 512, 512, 64, 64, 2, 1)
tp = pm.Dtd(ctx, "dead")
pm.insert_spd_fill(tp, A, 1)
pm.insert_potrf(tp, A)   # needs rank 1's tiles -> transfers hang -> EOF
tp.wait()
print("SHOULD_NOT_FINISH")
"""
    code_victim = f"""
import os, sys, time
sys.path.insert(0, {os.path.dirname(HERE)!r})
import parsec_amd as pm
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=1, world=2, comm="tcp", gpu=-2)
time.sleep(1.0)
os._exit(17)   # die without teardown, mid-protocol
"""
    port = _next_port[0]
    _next_port[0] += 4
    env = dict(os.environ)
    env.update(WORLD_SIZE="2", PORT=str(port))
    pa = subprocess.Popen([sys.executable, "-c", code_survivor], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    pb = subprocess.Popen([sys.executable, "-c", code_victim], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    ob, _ = pb.communicate(timeout=60)
    assert pb.returncode != 0  # victim died (17, or reset-abort if the
    # teardown race killed it first — incidental either way)
    oa, _ = pa.communicate(timeout=60)  # must NOT hang
    assert pa.returncode != 0 and b"SHOULD_NOT_FINISH" not in oa, oa.decode()
    assert b"connection to rank" in oa or b"FATAL" in oa, oa.decode()


def test_recv_copy_renaming(tmp_path):
    """An incoming version must not WAR-wait on readers of the previous
    version: the engine renames the tile to a fresh copy (datarepo/arena
    semantics, datarepo.h:25-92). Rank 1 rewrites a rank-0 tile each round
    while rank 0 holds a slow reader of the previous version; every reader
    must see exactly its version's value, the stale python handle must stay
    usable across renames, and the renames counter must engage."""
    import conftest
    REPO = os.path.dirname(HERE)
    port = str(conftest.port_base(13))
    code = """
import os, sys, time
sys.path.insert(0, %r)
import numpy as np
import parsec_amd as pm
rank = int(os.environ["RANK"])
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=2, comm="tcp", gpu=-2)
nb = 32
A = pm.TiledMatrix(ctx, 2 * nb, nb, nb, nb, 2, 1)
tp = pm.Dtd(ctx)
t00 = A.tile(0, 0)   # held across renames on purpose
seen = []
ROUNDS = 12
for k in range(ROUNDS):
    def w(buf, k=k):
        np.frombuffer(buf, dtype=np.float64)[:] = k + 1
    tp.insert_py(w, [(t00, pm.ACCESS_OUT)], rank=1, with_data=True)
    def r(buf, k=k):
        seen.append((k, float(np.frombuffer(buf, dtype=np.float64)[0])))
        time.sleep(0.02)  # hold the old version while the next recv lands
    tp.insert_py(r, [(t00, pm.ACCESS_IN)], rank=0, with_data=True)
tp.wait()
if rank == 0:
    assert len(seen) == ROUNDS, seen
    for k, v in seen:
        assert v == k + 1, (k, v)
    c = ctx.counters()
    assert c["renames"] > 0, c  # renaming actually engaged
    print("RENAME_OK", c["renames"])
ctx.barrier()
del A, ctx
""" % (REPO,)
    import subprocess as sp
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE="2", PORT=port)
        procs.append(sp.Popen([sys.executable, "-c", code], env=env,
                              stdout=sp.PIPE, stderr=sp.STDOUT))
    outs = []
    for pr in procs:
        o, _ = pr.communicate(timeout=180)
        outs.append(o)
        assert pr.returncode == 0, o.decode()
    assert b"RENAME_OK" in outs[0], outs[0].decode()


@pytest.mark.parametrize("world,p,q", [(4, 2, 2), (8, 2, 4)])
def test_distributed_cholesky_binomial_tree(world, p, q, tmp_path,
                                            monkeypatch):
    """Collective propagation tree (remote_dep.c:322-437 analog): panel
    fan-out re-sent through earlier recipients. Same numerics contract as
    the unicast run."""
    monkeypatch.setenv("PARSEC_MCA_bcast_tree", "binomial")
    pre, post = run_world(world, tmp_path, p, q)
    M = np.tril(pre) + np.tril(pre, -1).T
    L0 = np.linalg.cholesky(M)
    err = np.abs(np.tril(post) - L0).max()
    assert err < 1e-10, f"binomial world={world}: max err {err}"


def test_comm_peer_stats(tmp_path):
    """Per-peer comm counters (device-stats analog): bytes move in both
    directions and the table is per-peer."""
    import conftest
    REPO = os.path.dirname(HERE)
    port = str(conftest.port_base(17))
    code = """
import os, sys
sys.path.insert(0, %r)
import numpy as np
import parsec_amd as pm
rank = int(os.environ["RANK"])
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=2, comm="tcp", gpu=-2)
nb = 32
A = pm.TiledMatrix(ctx, 2 * nb, nb, nb, nb, 2, 1)
tp = pm.Dtd(ctx)
t00 = A.tile(0, 0)
for k2 in range(4):
    def w(buf, k2=k2):
        np.frombuffer(buf, dtype=np.float64)[:] = k2
    tp.insert_py(w, [(t00, pm.ACCESS_OUT)], rank=k2 %% 2, with_data=True)
    def r(buf):
        pass
    tp.insert_py(r, [(t00, pm.ACCESS_IN)], rank=(k2 + 1) %% 2,
                 with_data=True)
tp.wait()
st = ctx.comm_stats()
assert len(st) == 2
other = 1 - rank
assert st[other]["sent_bytes"] > 0 and st[other]["recv_bytes"] > 0, st
assert st[rank]["sent_bytes"] == 0 and st[rank]["recv_bytes"] == 0, st
print("PEERSTATS_OK", st[other])
ctx.barrier()
del A, ctx
""" % (REPO,)
    import subprocess as sp
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE="2", PORT=port)
        procs.append(sp.Popen([sys.executable, "-c", code], env=env,
                              stdout=sp.PIPE, stderr=sp.STDOUT))
    for pr in procs:
        o, _ = pr.communicate(timeout=180)
        assert pr.returncode == 0 and b"PEERSTATS_OK" in o, o.decode()


def test_ctl_messages_dynamic_insertion(tmp_path):
    """Control-message path (active-message seed, parsec_comm_engine.h AM
    tags analog): rank 0 discovers work at runtime and activates tasks on
    every other rank via tagged control messages — the non-SPMD pattern the
    deterministic dataflow protocol alone cannot express."""
    import conftest
    REPO = os.path.dirname(HERE)
    port = str(conftest.port_base(21))
    code = """
import os, sys, time, threading, queue
sys.path.insert(0, %r)
import numpy as np
import parsec_amd as pm
rank = int(os.environ["RANK"])
world = 4
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=world, comm="tcp", gpu=-2)
inbox = queue.Queue()
ctx.set_ctl_handler(lambda src, tag, payload: inbox.put((src, tag, payload)))
A = pm.TiledMatrix(ctx, 32 * world, 32, 32, 32, world, 1)
tp = pm.Dtd(ctx)
if rank != 0:
    if A.is_local(rank, 0):
        A.tile_numpy_set(rank, 0, np.zeros((32, 32)))
results = []
if rank == 0:
    # runtime "discovery": instruct each peer to run a local task with a
    # payload-carried operand, then collect their acks
    for dst in range(1, world):
        pm_payload = str(100 + dst).encode()
        ctx.send_ctl(dst, 7, pm_payload)
    acks = set()
    while len(acks) < world - 1:
        src, tag, payload = inbox.get(timeout=60)
        assert tag == 9
        acks.add((src, payload))
    vals = sorted(int(p) for _, p in acks)
    assert vals == [100 + d for d in range(1, world)], vals
    print("CTL_OK", vals)
else:
    src, tag, payload = inbox.get(timeout=60)
    assert src == 0 and tag == 7
    val = float(payload)
    t = A.tile(rank, 0)
    def body(buf, val=val):
        np.frombuffer(buf, dtype=np.float64)[:] = val
    tp.insert_py(body, [(t, pm.ACCESS_OUT)], rank=rank, with_data=True)
    tp.wait()
    got = A.tile_numpy(rank, 0)[0, 0]
    ctx.send_ctl(0, 9, str(int(got)).encode())
ctx.barrier()
del A, ctx
""" % (REPO,)
    import subprocess as sp
    procs = []
    for r in range(4):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE="4", PORT=port)
        procs.append(sp.Popen([sys.executable, "-c", code], env=env,
                              stdout=sp.PIPE, stderr=sp.STDOUT))
    outs = []
    for pr in procs:
        o, _ = pr.communicate(timeout=180)
        outs.append(o)
        assert pr.returncode == 0, o.decode()
    assert b"CTL_OK" in outs[0], outs[0].decode()


def test_wait_dynamic_token_ring(tmp_path):
    """Dynamic termination detection (mca/termdet fourcounter analog):
    a control-message token ring activates tasks on whichever rank holds
    the token — no rank knows its task count up front — and
    Taskpool.wait_dynamic() must terminate exactly when the ring quiesces."""
    import conftest
    REPO = os.path.dirname(HERE)
    port = str(conftest.port_base(29))
    code = """
import os, sys
sys.path.insert(0, %r)
import numpy as np
import parsec_amd as pm
rank = int(os.environ["RANK"])
world = 4
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=world, comm="tcp", gpu=-2)
A = pm.TiledMatrix(ctx, 32 * world, 32, 32, 32, world, 1)
if A.is_local(rank, 0):
    A.tile_numpy_set(rank, 0, np.zeros((32, 32)))
tp = pm.Dtd(ctx)
LAPS = 3
def on_token(src, tag, payload):
    hops = int(payload)
    t = A.tile(rank, 0)
    def body(buf, hops=hops):
        np.frombuffer(buf, dtype=np.float64)[:] += 1
        nxt = (rank + 1) %% world
        if hops > 1:
            ctx.send_ctl(nxt, 5, str(hops - 1).encode())
    tp.insert_py(body, [(t, pm.ACCESS_INOUT)], rank=rank, with_data=True)
ctx.set_ctl_handler(on_token)
if rank == 0:
    on_token(0, 5, str(LAPS * world).encode())
tp.wait_dynamic()
got = A.tile_numpy(rank, 0)[0, 0] if A.is_local(rank, 0) else None
assert got == LAPS, (rank, got)
print("TDYN_OK", rank, got)
ctx.barrier()
del A, ctx
""" % (REPO,)
    import subprocess as sp
    procs = []
    for r in range(4):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE="4", PORT=port)
        procs.append(sp.Popen([sys.executable, "-c", code], env=env,
                              stdout=sp.PIPE, stderr=sp.STDOUT))
    for pr in procs:
        o, _ = pr.communicate(timeout=180)
        assert pr.returncode == 0 and b"TDYN_OK" in o, o.decode()


def test_distributed_posv(tmp_path):
    """World-2 Cholesky factor+solve (insert_posv) over the TCP engine:
    the distributed solution matches numpy on the assembled system."""
    world, n, nb, nrhs = 2, 256, 64, 64
    port = _next_port[0]
    _next_port[0] += world + 2
    code = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["PARSEC_REPO"])
import parsec_amd as pm
rank = int(os.environ["RANK"])
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=2, comm="tcp", gpu=-2)
n, nb, nrhs = 256, 64, 64
A = pm.TiledMatrix(ctx, n, n, nb, nb, 2, 1, sym=True)
B = pm.TiledMatrix(ctx, n, nrhs, nb, nb, 2, 1)
tp = pm.Dtd(ctx)
pm.insert_spd_fill(tp, A, 11)
pm.insert_full_fill(tp, B, 5)
tp.wait()
pre = {}
for i in range(A.mt):
    for j in range(i + 1):
        if A.is_local(i, j):
            pre[f"a_{i}_{j}"] = A.tile_numpy(i, j)
    if B.is_local(i, 0):
        pre[f"b_{i}_0"] = B.tile_numpy(i, 0)
tp2 = pm.Dtd(ctx)
pm.insert_posv(tp2, A, B)
tp2.wait()
tp2.flush_all(B)
post = {}
for i in range(B.mt):
    if B.is_local(i, 0):
        post[f"x_{i}_0"] = B.tile_numpy(i, 0)
np.savez(os.path.join(os.environ["OUT"], f"posv{rank}.npz"), **pre, **post)
ctx.barrier()
del A, B, tp, tp2, ctx
print("POSV_RANK_OK", rank)
"""
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world), PORT=str(port),
                   OUT=str(tmp_path),
                   PARSEC_REPO=os.path.dirname(HERE))
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env,
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for pr in procs:
        out, _ = pr.communicate(timeout=180)
        assert pr.returncode == 0 and b"POSV_RANK_OK" in out, out.decode()
    Af = np.zeros((n, n))
    Bf = np.zeros((n, nrhs))
    X = np.zeros((n, nrhs))
    for r in range(world):
        z = np.load(os.path.join(tmp_path, f"posv{r}.npz"))
        for key in z.files:
            kind, i, j = key.split("_")
            i, j = int(i), int(j)
            if kind == "a":
                Af[i * nb:(i + 1) * nb, j * nb:(j + 1) * nb] = z[key]
            elif kind == "b":
                Bf[i * nb:(i + 1) * nb, :] = z[key]
            else:
                X[i * nb:(i + 1) * nb, :] = z[key]
    Lo = np.tril(Af)
    Af = Lo + np.tril(Lo, -1).T
    ref = np.linalg.solve(Af, Bf)
    err = np.abs(X - ref).max() / np.abs(ref).max()
    assert err < 1e-11, f"distributed posv rel err {err}"


def test_ctl_self_send_loopback(tmp_path):
    """send_ctl(dst == my rank) loops back through the comm thread: apps
    with computed destinations (dynamic token patterns) may land on
    themselves, and the termdet counters must balance exactly as for a
    remote delivery (wait_dynamic below would hang on an imbalance)."""
    import conftest
    REPO = os.path.dirname(HERE)
    port = str(conftest.port_base(33))
    code = r"""
import os, sys
sys.path.insert(0, os.environ["PARSEC_REPO"])
import numpy as np
import parsec_amd as pm
rank = int(os.environ["RANK"])
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=2, comm="tcp", gpu=-2)
A = pm.TiledMatrix(ctx, 64, 32, 32, 32, 2, 1)
if A.is_local(rank, 0):
    A.tile_numpy_set(rank, 0, np.zeros((32, 32)))
tp = pm.Dtd(ctx)
def on_token(src, tag, payload):
    b = int(payload)
    def body(buf):
        np.frombuffer(buf, dtype=np.float64)[:] += 1
    tp.insert_py(body, [(A.tile(rank, 0), pm.ACCESS_INOUT)], rank=rank,
                 with_data=True)
    if b > 1:
        # alternate SELF and peer: half the hops are loopbacks
        dst = rank if b % 2 == 0 else 1 - rank
        ctx.send_ctl(dst, 5, str(b - 1).encode())
if rank == 0:
    pass
ctx.set_ctl_handler(on_token)
if rank == 0:
    on_token(0, 5, b"12")
tp.wait_dynamic()
mine = int(A.tile_numpy(rank, 0)[0, 0]) if A.is_local(rank, 0) else 0
print("SELF_OK", rank, mine)
ctx.barrier()
del A, ctx
"""
    procs = []
    total = 0
    for r in range(2):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE="2", PORT=port,
                   PARSEC_REPO=REPO)
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env,
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for pr in procs:
        out, _ = pr.communicate(timeout=120)
        assert pr.returncode == 0 and b"SELF_OK" in out, out.decode()
        for line in out.decode().splitlines():
            if line.startswith("SELF_OK"):
                total += int(line.split()[2])
    assert total == 12, total


def test_wait_dynamic_random_split(tmp_path):
    """Randomized dynamic-activation fuzz (the pattern that found the
    ctl self-send gap): each token inserts one task and randomly splits
    its remaining budget across random ranks (self included). Budget
    conservation makes the global task count exactly K; wait_dynamic
    must neither hang nor return early (sum of counters < K)."""
    import conftest
    REPO = os.path.dirname(HERE)
    code = r"""
import os, sys, random
sys.path.insert(0, os.environ["PARSEC_REPO"])
import numpy as np
import parsec_amd as pm
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
seed = int(os.environ["SEED"]); K = int(os.environ["K"])
pm.param_set("comm_base_port", os.environ["PORT"])
ctx = pm.Context(nworkers=2, rank=rank, world=world, comm="tcp", gpu=-2)
A = pm.TiledMatrix(ctx, 32 * world, 32, 32, 32, world, 1)
if A.is_local(rank, 0):
    A.tile_numpy_set(rank, 0, np.zeros((32, 32)))
tp = pm.Dtd(ctx)
rng = random.Random(seed * 1000 + rank)
def on_token(src, tag, payload):
    b = int(payload)
    def body(buf):
        np.frombuffer(buf, dtype=np.float64)[:] += 1
    tp.insert_py(body, [(A.tile(rank, 0), pm.ACCESS_INOUT)], rank=rank,
                 with_data=True)
    rest = b - 1
    if rest > 0:
        parts = [rest]
        if rest > 1 and rng.random() < 0.5:
            cut = rng.randrange(1, rest)
            parts = [cut, rest - cut]
        for p in parts:
            ctx.send_ctl(rng.randrange(world), 5, str(p).encode())
ctx.set_ctl_handler(on_token)
if rank == 0:
    on_token(0, 5, str(K).encode())
tp.wait_dynamic()
mine = int(A.tile_numpy(rank, 0)[0, 0]) if A.is_local(rank, 0) else 0
print("TDYNF", rank, mine)
ctx.barrier()
del A, ctx
"""
    for seed in (3007, 3013):
        port = _next_port[0]
        _next_port[0] += 6
        procs = []
        for r in range(4):
            env = dict(os.environ)
            env.update(RANK=str(r), WORLD_SIZE="4", PORT=str(port),
                       SEED=str(seed), K="150", PARSEC_REPO=REPO)
            procs.append(subprocess.Popen([sys.executable, "-c", code],
                                          env=env, stdout=subprocess.PIPE,
                                          stderr=subprocess.STDOUT))
        total = 0
        for pr in procs:
            out, _ = pr.communicate(timeout=120)
            assert pr.returncode == 0, out.decode()
            for line in out.decode().splitlines():
                if line.startswith("TDYNF"):
                    total += int(line.split()[2])
        assert total == 150, (seed, total)
