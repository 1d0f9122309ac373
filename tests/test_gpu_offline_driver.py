"""GPU tests of the multi-GPU offline driver (gnn-pe_amd/offline.py): for 1, 2 and 3 ranks the files are
byte-identical to the reference's (golden md5s), index.dat satisfies the consumer's constraints, and the
untouched reference `main -m online` prints the known answer.  The box has one GPU, so ranks > 1 share
device 0 and their collectives run over gloo (GNNPE_BENCH_SAME_DEVICE=1); the slab partition, halo
exchange, output assembly and index gather are the production code paths."""
import hashlib
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gnnpe_amd import synth
from oracle import ref_main_path

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gnn-pe_amd", "offline.py")


def _md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [1, 2, 3])
def test_driver_files_match_reference_for_any_world_size(tmp_path, oracle, world):
    gold = json.load(open(os.path.join(GOLDEN, "test_graph", "golden.json")))["p2"]
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    deg = np.array([int(l.split()[3]) for l in open(graph) if l.startswith("v")])
    sn = np.argsort(deg, kind="stable").astype(np.uint32)
    tmp = str(tmp_path)
    synth.make_dataset_dir(tmp, 2)
    synth.write_membership(os.path.join(tmp, "gnn-pe", "membership.txt"), sn, (np.arange(len(deg)) % 2).astype(np.uint32))
    args = [DRIVER, "-f", tmp + "/", "-d", graph, "-p", "2", "--index", "--chunk", "60000"]
    env = dict(os.environ)
    if world == 1:
        cmd = [sys.executable] + args
    else:
        env["GNNPE_BENCH_SAME_DEVICE"] = "1"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "|V|: 3112, |E|: 12519, |Σ|: 71" in r.stdout
    assert _md5(os.path.join(tmp, "gnn-pe", "all_paths.txt")) == gold["all_paths_md5"]
    for i in range(2):
        d = os.path.join(tmp, "gnn-pe", "partitions", f"partition-{i}")
        assert _md5(os.path.join(d, "partition_paths.txt")) == gold["partition_paths_md5"][i]
        info = oracle.index_validate(open(os.path.join(d, "index.dat"), "rb").read())
        assert info["num_data"] == gold["partition_sizes"][i]
        assert np.array_equal(np.sort(info["leaf_son"]), np.arange(gold["partition_sizes"][i]))
    if world == 3 and os.path.exists(ref_main_path()):
        out = subprocess.check_output([ref_main_path(), "-f", tmp + "/", "-d", graph, "-q",
                                       os.path.join(GOLDEN, "test_graph", "query_graph.graph"), "-m", "online", "-p", "2"],
                                      text=True)
        assert int(re.search(r"Answer Number: (\d+)", out).group(1)) == gold["answer_number"] == 45426


@pytest.mark.parametrize("world", [1, 2])
def test_driver_l3_two_hop_halo(tmp_path, oracle, world):
    """-l 3 through the rank-partitioned driver: the second halo round brings in the rows two hops from the slab;
    files equal the oracle writers over the fixed-depth DFS (no reference run exists for l=3), and the
    4-vertex index.dat satisfies the format validator."""
    g = synth.gnm_graph(500, 1900, n_labels=5, seed=77)
    rng = np.random.default_rng(77)
    sn = rng.permutation(500).astype(np.uint32)
    mem = rng.integers(0, 2, size=500).astype(np.uint32)
    tmp = str(tmp_path / "ds")
    os.makedirs(tmp)
    synth.make_dataset_dir(tmp, 2)
    synth.write_membership(os.path.join(tmp, "gnn-pe", "membership.txt"), sn, mem)
    gp = str(tmp_path / "g.graph")
    synth.write_graph_file(gp, g)
    args = [DRIVER, "-f", tmp + "/", "-d", gp, "-p", "2", "-l", "3", "--index", "--chunk", "20000"]
    env = dict(os.environ)
    if world == 1:
        cmd = [sys.executable] + args
    else:
        env["GNNPE_BENCH_SAME_DEVICE"] = "1"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    want = oracle.enumerate_dfs_hash(g["offsets"], g["nbrs"], sn, 4)
    assert open(os.path.join(tmp, "gnn-pe", "all_paths.txt"), "rb").read() == oracle.format_all_paths(want)
    for pid in range(2):
        d = os.path.join(tmp, "gnn-pe", "partitions", f"partition-{pid}")
        exp = str(tmp_path / f"exp{pid}.txt")
        oracle.write_partition_paths(exp, want, mem, pid)
        assert open(os.path.join(d, "partition_paths.txt"), "rb").read() == open(exp, "rb").read()
        info = oracle.index_validate(open(os.path.join(d, "index.dat"), "rb").read())
        cnt = int((mem[want[:, 0]] == pid).sum())
        assert info["num_data"] == cnt and info["dim"] == 8
        assert np.array_equal(np.sort(info["leaf_son"]), np.arange(cnt))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_driver_answers_a_query_across_ranks(tmp_path, world):
    """online side over the slab-partitioned graph: per-rank filter, bitmaps OR-ed (all-reduce), refinement on rank 0
    -> the reference's answer count for its sample query"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    query = os.path.join(GOLDEN, "test_graph", "query_graph.graph")
    deg = np.array([int(l.split()[3]) for l in open(graph) if l.startswith("v")])
    tmp = str(tmp_path)
    synth.make_dataset_dir(tmp, 1)
    synth.write_membership(os.path.join(tmp, "gnn-pe", "membership.txt"), np.argsort(deg, kind="stable").astype(np.uint32),
                           np.zeros(len(deg), np.uint32))
    args = [DRIVER, "-f", tmp + "/", "-d", graph, "-p", "1", "-q", query]
    env = dict(os.environ)
    if world == 1:
        cmd = [sys.executable] + args
    else:
        env["GNNPE_BENCH_SAME_DEVICE"] = "1"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(re.search(r"Answer Number: (\d+)", r.stdout).group(1)) == 45426


def test_bench_multi_rank_flow_on_one_device(tmp_path):
    """bench.py's N > 1 path (slab planning, load_rows, halo install, per-step vde all-gather / count all-gather / fill,
    the closed-form sanity check, max-over-ranks timing) with two ranks sharing device 0 over gloo
    (GNNPE_BENCH_SAME_DEVICE=1: the explicit debugging mode; the driver's own runs use RCCL, one GPU per rank)."""
    import json
    env = dict(os.environ, GNNPE_BENCH_SAME_DEVICE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--vertices", "200000", "--edges", "2000000", "--placements", "1", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "slab2" and d["scaling"] == "strong"
    assert d["config"]["paths"] == synth.expected_paths_l2(synth.gnm_graph(200_000, 2_000_000)["offsets"])
    assert d["value"] > 0 and d["halo"]["halo_rows"] > 0 and "halo_install_ms" in d["phases_ms"]["one_time"]
    assert d["cpu_baseline"] is None and "gloo" in d["config"]["collectives"]
