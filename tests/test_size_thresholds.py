"""The launch-shape constants that tests/test_size_thresholds_gpu.py was sized for, read from the sources: if a cap moves, this
test fails instead of the large-input coverage silently turning into small-input coverage.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source file, name) -> the value the GPU tests' shapes were chosen for
SIZED_FOR = {
    ("v2e_amd/csrc/denoise.hip", "AGES_MAX_BLOCKS"): 2048,        # x 256 threads: a second grid-stride trip above 524 288 valid rows
    ("v2e_amd/csrc/patches.hip", "FEATURES_MAX_BLOCKS"): 65536,   # x 256: above 16 777 216 (row, offset) items
    ("v2e_amd/csrc/tensorize.hip", "SCATTER_MAX_BLOCKS"): 4096,   # x 256: above 1 048 576 rows
    ("v2e_amd/csrc/tensorize.hip", "LDS_BOUNDS_MAX"): 4096,       # explicit bounds in LDS up to this many entries
    ("v2e_amd/csrc/sinks.hip", "P32_BLOCK"): 1024,                # rows per workgroup of pack32; k_pack32_scan: 1024 threads
    ("include/v2e_amd.h", "V2E_READER_BLOCK"): 1024,              # records per workgroup of the readers; k_rd_scan: 1024 threads
    ("v2e_amd/csrc/readers.hip", "NL_BYTES"): 16,                 # x V2E_READER_BLOCK: bytes per workgroup of the newline passes
    ("v2e_amd/csrc/readers.hip", "LINE_BLOCK"): 256,              # lines per workgroup of the parse pass
}
AGES_ITEMS = 2048 * 256
FEATURES_ITEMS = 65536 * 256
SCATTER_ROWS = 4096 * 256
LDS_BOUNDS_MAX = 4096
SCAN_THREADS = 1024
P32_BLOCK = 1024
READER_BLOCK = 1024
NL_BLOCK_BYTES = 1024 * 16
LINE_BLOCK = 256


def _constant(path, name):
    src = open(os.path.join(ROOT, path)).read()
    m = re.findall(r"^\s*(?:constexpr int %s =|#define %s) ([0-9 <]+?)\s*;?\s*(?://.*|/\*.*)?$" % (name, name), src, flags=re.M)
    assert len(m) == 1, (path, name, m)
    expr = m[0].strip()
    if "<<" in expr:
        a, b = expr.split("<<")
        return int(a) << int(b)
    return int(expr)


def test_launch_shape_constants_are_what_the_size_tests_were_sized_for():
    assert {k: _constant(*k) for k in SIZED_FOR} == SIZED_FOR
    assert (AGES_ITEMS, FEATURES_ITEMS, SCATTER_ROWS) == (SIZED_FOR["v2e_amd/csrc/denoise.hip", "AGES_MAX_BLOCKS"] * 256,
                                                          SIZED_FOR["v2e_amd/csrc/patches.hip", "FEATURES_MAX_BLOCKS"] * 256,
                                                          SIZED_FOR["v2e_amd/csrc/tensorize.hip", "SCATTER_MAX_BLOCKS"] * 256)
    src = {p: open(os.path.join(ROOT, p)).read() for p in set(k[0] for k in SIZED_FOR)}
    # the block size (256) and the scan width (1024) the products above assume, where the launches say them
    assert "k_denoise_ages<<<(int)(blocks < AGES_MAX_BLOCKS ? blocks : AGES_MAX_BLOCKS), 256," in src["v2e_amd/csrc/denoise.hip"]
    assert "want < FEATURES_MAX_BLOCKS ? want : FEATURES_MAX_BLOCKS" in src["v2e_amd/csrc/patches.hip"]
    assert "const int64_t want = (n * PP + 255) / 256;" in src["v2e_amd/csrc/patches.hip"]
    assert "k_tensorize_scatter<<<(int)(blocks < SCATTER_MAX_BLOCKS ? blocks : SCATTER_MAX_BLOCKS), 256," in src["v2e_amd/csrc/tensorize.hip"]
    assert "k_pack32_scan<<<1, 1024, 0, s>>>" in src["v2e_amd/csrc/sinks.hip"]
    assert src["v2e_amd/csrc/readers.hip"].count("k_rd_scan<<<1, 1024, 0, s>>>") == 3
    assert "constexpr int RB = V2E_READER_BLOCK;" in src["v2e_amd/csrc/readers.hip"]
    assert "constexpr int NL_BLOCK_BYTES = RB * NL_BYTES;" in src["v2e_amd/csrc/readers.hip"]
    from v2e_amd import readers
    from v2e_amd.denoise import DEFAULT_ROWS_PER_PASS
    assert readers.READER_BLOCK == READER_BLOCK and DEFAULT_ROWS_PER_PASS > 2 * 1024 * 1024
