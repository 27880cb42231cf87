"""mmseq -pairs without a device: the flags and their refusals, and the pair generation of host/pairs_gen.hpp through its stand-alone
driver against a restatement of the rule."""
import os
import subprocess
from itertools import combinations

from oracle import host_oracle as H
from test_cli import BIN_DIR, dataset, run

PAIRS_GEN = os.path.join(BIN_DIR, "pairs_gen_test")


def test_usage_and_flag_refusals():
    r = run(["-help"])
    assert r.returncode == 1 and b"\n  -pairs " in r.stderr and b"\n  -pairs_maxset INT" in r.stderr and b".pairs" in r.stderr
    r = run(["-pairs", "-gpus", "2", "a", "b"])
    assert r.returncode == 1 and b"Error: -pairs reads the chain's trace on one device: it cannot be combined with -gpus > 1." in r.stderr
    assert b"no HIP device available" not in r.stderr
    for v in ("1", "0", "-3"):
        r = run(["-pairs", "-pairs_maxset", v, "a", "b"])
        assert r.returncode == 1 and b"Error: -pairs_maxset must be at least 2." in r.stderr and b"no HIP device available" not in r.stderr


def restate(rows, k, maxset, label=None):
    """{(a, b): [shared_hits, shared_sets]} with a < b, and the skipped sets with their hits"""
    pairs, skipped = {}, [0, 0]
    for row, ki in zip(rows, k):
        ts = sorted(set(int(t) if label is None else label[int(t)] for t in row))
        if len(row) > maxset:
            skipped[0] += 1; skipped[1] += int(ki)
            continue
        for a, b in combinations(ts, 2):
            e = pairs.setdefault((a, b), [0, 0])
            e[0] += int(ki); e[1] += 1
    return pairs, skipped


def generate(tmp_path, rows, k, maxset):
    f = tmp_path / "sets.txt"
    f.write_text("".join("%d %s\n" % (ki, " ".join(str(int(t)) for t in row)) for row, ki in zip(rows, k)))
    r = subprocess.run([PAIRS_GEN, str(f), str(maxset)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    lines = r.stdout.decode().split("\n")
    assert lines[-1] == ""
    last = lines[-2].split(" ")
    assert last[0] == "skipped_sets" and last[2] == "skipped_hits"
    got = [tuple(int(v) for v in ln.split(" ")) for ln in lines[:-2]]
    return got, [int(last[1]), int(last[3])]


def test_pair_generation_on_a_hand_written_case(tmp_path):
    maxset = 4
    rows = [[7],                       # a set of one: no pair
            [3, 1], [1, 3], [1, 2, 3],  # the pair (1, 3) in three sets with different k, members unsorted in the first
            [9, 2, 5, 0],              # exactly maxset, unsorted: six pairs
            [0, 1, 2, 3, 4],           # maxset + 1: skipped and counted
            [10, 11, 12, 13, 14, 15],  # longer still
            [5, 9]]
    k = [4, 10, 7, 1, 3, 9, 2, 6]
    got, skipped = generate(tmp_path, rows, k, maxset)
    want = [(0, 2, 3, 1), (0, 5, 3, 1), (0, 9, 3, 1), (1, 2, 1, 1), (1, 3, 18, 3), (2, 3, 1, 1), (2, 5, 3, 1), (2, 9, 3, 1), (5, 9, 9, 2)]
    assert got == want and skipped == [2, 11]
    ref, ref_skipped = restate(rows, k, maxset)
    assert got == [(a, b, v[0], v[1]) for (a, b), v in sorted(ref.items())] and skipped == ref_skipped
    # maxset 2: only the sets of two are left
    got2, skipped2 = generate(tmp_path, rows, k, 2)
    assert got2 == [(1, 3, 17, 2), (5, 9, 6, 1)] and skipped2 == [4, 15]
    # below 2: refused
    f = tmp_path / "sets.txt"
    r = subprocess.run([PAIRS_GEN, str(f), "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and b"at least 2" in r.stderr and r.stdout == b""


def test_pair_generation_on_the_cli_datasets_hit_sets(tmp_path):
    g = H.ingest(dataset(n_reads=1500))
    for maxset, n_pairs, n_skipped in ((16, 160, 0), (3, 136, 93)):
        got, skipped = generate(tmp_path, g["rows"], g["k"], maxset)
        ref, ref_skipped = restate(g["rows"], g["k"], maxset)
        assert got == [(a, b, v[0], v[1]) for (a, b), v in sorted(ref.items())]
        assert skipped == ref_skipped and len(got) == n_pairs and skipped[0] == n_skipped
        assert all(a < b for a, b, _, _ in got) and got == sorted(got)
