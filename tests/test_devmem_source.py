"""Device memory has one owner, hkc::DevBuf (hakai-fem_amd/csrc/hakai_devmem.hpp): no other source of
the library calls the runtime's allocator, and the raw helpers it replaced are gone (CPU; the sources
are read, nothing is compiled)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hakai-fem_amd", "csrc")
OWNER = "hakai_devmem.hpp"


def _sources():
    files = sorted(f for ext in ("hip", "cpp", "hpp") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) >= 30 and os.path.join(CSRC, OWNER) in files
    return {os.path.basename(f): open(f).read() for f in files}


def _where(pattern):
    return sorted(name for name, text in _sources().items() if re.search(pattern, text))


def test_only_the_owner_calls_the_allocator():
    assert _where(r"\bhipMalloc\(") == [OWNER]
    assert _where(r"\bhipFree\(") == [OWNER]


def test_the_raw_helpers_are_gone():
    assert _where(r"\bdalloc\(") == []
    assert _where(r"\bdfree\(") == []
