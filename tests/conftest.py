"""Shared fixtures. Tests marked `gpu` need a gfx950 device (run on the MI355X box); everything
else runs on CPU. The oracle (oracle/) is imported only here in tests, as the checker.

GPU test order: the BASELINE configurations and the reference's own decks run first (C2/C4/C5 in
test_gpu_configs, C3 in test_gpu_fullsize, C1 and the decks in test_gpu_exact / test_gpu_decks /
test_gpu_parity), so a `-x` stop in a later, narrower test cannot hide them."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hakai-fem_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DECKS_GOLDEN = os.path.join(ROOT, "tests", "golden", "decks")

_FIRST = ("test_gpu_exact.py", "test_gpu_configs.py", "test_gpu_fullsize.py", "test_gpu_decks.py",
          "test_gpu_parity.py")
_LAST = ("test_gpu_own.py", "test_gpu_multirank.py", "test_gpu_rccl.py")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a gfx950 (MI355X) GPU")
    config.addinivalue_line("markers", "slow: long-running")


def pytest_collection_modifyitems(config, items):
    def rank(item):
        f = os.path.basename(str(item.fspath))
        if f in _FIRST:
            return _FIRST.index(f)
        if f in _LAST:
            return 100 + _LAST.index(f)
        return 50
    items.sort(key=rank)  # stable: file order within a rank, test order within a file


@pytest.fixture(scope="session")
def ref_decks(tmp_path_factory):
    """The reference's input decks (v0.0.0-v0.0.2), stored gzipped under tests/golden/decks in the
    reference's own layout (HAKAI-v0.0.x/input/<deck>.inp.gz), unpacked once per session. Returns
    the directory that holds the HAKAI-v0.0.x folders."""
    import gzip
    import shutil
    out = tmp_path_factory.mktemp("reference_decks")
    for d, _, files in os.walk(DECKS_GOLDEN):
        for f in sorted(files):
            if not f.endswith(".inp.gz"):
                continue
            dst = out / os.path.relpath(d, DECKS_GOLDEN)
            dst.mkdir(parents=True, exist_ok=True)
            with gzip.open(os.path.join(d, f), "rb") as src, open(dst / f[:-3], "wb") as fh:
                shutil.copyfileobj(src, fh)
    return str(out)


@pytest.fixture(scope="session")
def has_gpu():
    import hakai
    return hakai.device_count() > 0
