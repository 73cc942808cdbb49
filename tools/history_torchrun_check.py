#!/usr/bin/env python3
"""History output of the N-GPU driver over RCCL against the in-process group of the same partition:
writes a contact deck, runs hakai.run.hakai_multi(local_ranks=N) with HAKAI_HISTORY set, then
`python -m hakai.run` under torch.distributed.run with --nproc ranks (on a one-GPU box the ranks
share the device and RCCL connects them over loopback, hakai.dist.rank_device; this script sets
HAKAI_RCCL_SHARED_GPU=1 for its ranks), and compares the two history.csv files byte for byte: a
rank's record depends on the partition alone, not on the transport of the interface exchange, and
rank 0 combines the gathered records in rank order either way."""
import os
import socket
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hakai-fem_amd"), os.path.join(ROOT, "tests")]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--nproc", type=int, default=2)
    ap.add_argument("--stride", type=int, default=5)
    args = ap.parse_args()
    from hakai import mesh
    from hakai.run import hakai_multi
    from inp_writer import write_inp
    tmp = tempfile.mkdtemp(prefix="hakai_hist_")
    m = mesh.two_body_model(plate=(6, 6, 1), impactor=(2, 2, 3), v=-3e5, d_time=2e-8, n_steps=400)
    deck = write_inp(os.path.join(tmp, "impact.inp"), m)
    os.environ["HAKAI_HISTORY"] = str(args.stride)
    hakai_multi(deck, os.path.join(tmp, "local"), local_ranks=args.nproc, verbose=False)
    env = dict(os.environ, HAKAI_RCCL_SHARED_GPU="1",
               PYTHONPATH=os.path.join(ROOT, "hakai-fem_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.nproc),
                        "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m", "hakai.run", deck,
                        os.path.join(tmp, "rccl")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    if r.returncode:
        return r.returncode
    a = open(os.path.join(tmp, "local", "history.csv"), "rb").read()
    b = open(os.path.join(tmp, "rccl", "history.csv"), "rb").read()
    n = a.count(b"\n") - 1
    same = a == b and n == m.n_steps // args.stride
    print(f"torchrun driver (world {args.nproc}) vs in-process group: history.csv, {n} records, byte-identical: {same}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
