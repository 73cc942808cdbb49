"""History output of the N-GPU driver over RCCL (python -m hakai.run under torch.distributed.run, 2
ranks sharing the GPU as in test_gpu_rccl.py): its history.csv is byte-identical to the in-process
2-rank driver's for the same deck -- the record depends on the partition, not on the transport."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_torchrun_driver_writes_the_same_history_csv():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "history_torchrun_check.py"), "--nproc", "2"],
                       capture_output=True, text=True, timeout=400, cwd=ROOT,
                       env=dict(os.environ, HAKAI_RCCL_SHARED_GPU="1"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "history.csv, 80 records, byte-identical: True" in r.stdout
