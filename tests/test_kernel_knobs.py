"""The kernel library's environment knobs live in one table (hpgmg_amd/csrc/kernels/knobs.hip): name, default, accepted values.  A knob is read on its
first use, never when the library loads; a value outside the accepted set costs one line on stderr and gives the default.  No GPU: every case runs in a child
process that only dlopens the library and reads the table through the C ABI (include/hpgmg_hip.h: hpgmg_hip_knob_*) -- no launcher is called."""
import json
import os
import re
import subprocess
import sys

import pytest

from hpgmg_testlib import ROOT
from test_cabi_symbols import ensure_built

KERNELS = os.path.join(ROOT, "hpgmg_amd", "csrc", "kernels")

# every row and its default, in the table's order: a default cannot move unnoticed
ROWS = [
    ("HPGMG_TUNE_PAIR_PACKED", 1), ("HPGMG_TUNE_PAIR_KC", 0), ("HPGMG_TUNE_PAIR_NW", 0),
    ("HPGMG_TUNE_TY", 0), ("HPGMG_TUNE_KCHUNK", 0), ("HPGMG_TUNE_MIN_KCHUNK", 1), ("HPGMG_TUNE_WANT_BLOCKS", 4096),
    ("HPGMG_TUNE_27PT_TILE32", 0), ("HPGMG_TUNE_27PT_DIRECT", 0), ("HPGMG_TUNE_27PT_KCHUNK", 0),
    ("HPGMG_TUNE_FV4_TILE32", 1), ("HPGMG_TUNE_FV4_KCHUNK_MIN", 8), ("HPGMG_TUNE_FV4_KCHUNK", 0), ("HPGMG_TUNE_FV4_TJ", 8), ("HPGMG_TUNE_FV4_DIRECT", 0),
    ("HPGMG_TUNE_NO_WIDE", 0), ("HPGMG_TUNE_WIDE_WJ", 8), ("HPGMG_TUNE_7PT_NO_TILE", 0), ("HPGMG_TUNE_7PT_TILE_KCHUNK", 8), ("HPGMG_TUNE_SMALL_RR", 1),
    ("HPGMG_TUNE_27PT_NO_RB", 0), ("HPGMG_TUNE_27PT_RB_KCHUNK", 0), ("HPGMG_TUNE_27PT_NO_RB_BOX", 0), ("HPGMG_TUNE_27PT_RB_BOX_MAXDIM", 8),
    ("HPGMG_TUNE_FV4_NO_RB", 0), ("HPGMG_TUNE_FV4_RB_ORDER", 1), ("HPGMG_TUNE_FV4_RB_KCHUNK", 0), ("HPGMG_EXP_TIMELINE_WG", -1),
    ("HPGMG_TUNE_SMALL_NO_LDS", 0), ("HPGMG_TUNE_BOTTOM_THREADS", 512),
    ("HPGMG_TUNE_COPY_NT", 1), ("HPGMG_TUNE_INTERP_NT", 1),
    ("HPGMG_TEST_BRICK_CAPACITY", -1), ("HPGMG_TEST_BRICK_ABSENT", -1),
    ("HPGMG_RCCL_SUBCOMM", 1), ("HPGMG_IPC_DEBUG", 0), ("HPGMG_ROCTX", 0), ("HPGMG_GRAPH_DEBUG", 0),
]
DEFAULT = dict(ROWS)

# the child: argv[1] = the kernel library.  value(name) is the first read of that knob unless the body read it before.
PRELUDE = """
import ctypes, json, os, sys
K = ctypes.CDLL(sys.argv[1])
K.hpgmg_hip_knob_name.restype = ctypes.c_char_p
K.hpgmg_hip_knob_value.restype = ctypes.c_longlong
K.hpgmg_hip_knob_default.restype = ctypes.c_longlong
names = [K.hpgmg_hip_knob_name(i).decode() for i in range(K.hpgmg_hip_knob_count())]
def value(name): return K.hpgmg_hip_knob_value(names.index(name))
"""


def child(body, **env):
    """Run body after PRELUDE with no HPGMG_* variable set but those given; what it printed as JSON, and its stderr."""
    hip, _ = ensure_built()
    clean = {k: v for k, v in os.environ.items() if not k.startswith("HPGMG_")}
    out = subprocess.run([sys.executable, "-c", PRELUDE + body, hip], capture_output=True, text=True, timeout=60, env=dict(clean, **env))
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
    return json.loads(out.stdout), out.stderr


def test_every_row_has_its_default_when_nothing_is_set():
    rows, err = child("print(json.dumps([[n, K.hpgmg_hip_knob_default(i), K.hpgmg_hip_knob_value(i)] for i, n in enumerate(names)]))")
    assert [(n, d) for n, d, _ in rows] == ROWS
    assert all(v == d for _, d, v in rows)
    assert err == ""


@pytest.mark.parametrize("name,text", [("HPGMG_TUNE_PAIR_NW", "10"), ("HPGMG_TUNE_PAIR_NW", "12"), ("HPGMG_TUNE_PAIR_NW", "16"), ("HPGMG_TUNE_PAIR_KC", "3"),
                                       ("HPGMG_TUNE_PAIR_KC", "24"), ("HPGMG_TUNE_WIDE_WJ", "4"), ("HPGMG_TUNE_FV4_TJ", "16"), ("HPGMG_TEST_BRICK_CAPACITY", "100"),
                                       ("HPGMG_TUNE_COPY_NT", "0")])
def test_an_accepted_value_is_taken(name, text):
    got, err = child(f"print(json.dumps(value({name!r})))", **{name: text})
    assert got == int(text) and got != DEFAULT[name]
    assert err == ""


@pytest.mark.parametrize("name,text", [("HPGMG_TUNE_PAIR_NW", "11"), ("HPGMG_TUNE_WIDE_WJ", "3"), ("HPGMG_TUNE_WIDE_WJ", "16"), ("HPGMG_TUNE_TY", "3"),
                                       ("HPGMG_TUNE_MIN_KCHUNK", "0"), ("HPGMG_TUNE_FV4_KCHUNK_MIN", "0"), ("HPGMG_TUNE_NO_WIDE", "2"), ("HPGMG_TUNE_PAIR_KC", "abc"),
                                       ("HPGMG_TUNE_PAIR_KC", "-1")])
def test_a_refused_value_gives_the_default_and_one_line(name, text):
    """Each of these went through the old parse unchanged (pair.hip, stencil.hip: a division by zero, a launch shape no kernel instance has) or as atoi's 0."""
    got, err = child(f"print(json.dumps([value({name!r}), value({name!r})]))", **{name: text})
    assert got == [DEFAULT[name], DEFAULT[name]]
    lines = err.splitlines()
    assert len(lines) == 1, err
    assert lines[0].startswith(f"hpgmg_hip: {name}={text} is not accepted (") and lines[0].endswith(f"); using {DEFAULT[name]}"), err


def test_an_empty_string_is_the_default_silently():
    got, err = child("print(json.dumps([value(n) for n in names]))", **{n: "" for n, _ in ROWS})
    assert got == [d for _, d in ROWS]
    assert err == ""


def test_a_knob_is_read_on_first_use_not_at_load_time():
    got, err = child("os.environ['HPGMG_TUNE_PAIR_NW'] = '12'\nos.environ['HPGMG_TUNE_FV4_NO_RB'] = '1'\n"
                     "print(json.dumps([value('HPGMG_TUNE_PAIR_NW'), value('HPGMG_TUNE_FV4_NO_RB')]))")
    assert got == [12, 1]
    assert err == ""


def test_the_setters_write_the_table():
    got, err = child("K.hpgmg_hip_set_27pt_tile32(1)\nK.hpgmg_hip_set_27pt_rb_box_maxdim(32)\n"
                     "print(json.dumps([value('HPGMG_TUNE_27PT_TILE32'), value('HPGMG_TUNE_27PT_RB_BOX_MAXDIM')]))")
    assert got == [1, 32]
    assert err == ""


def test_no_other_environment_read_under_kernels():
    """One parse: getenv in knobs.hip, and once in comm_ipc.hip (HPGMG_IPC_TIMEOUT, a real number of seconds); the old helper is gone."""
    reads = {}
    for f in sorted(os.listdir(KERNELS)):
        text = open(os.path.join(KERNELS, f), errors="ignore").read()
        assert "env_int" not in text, f
        if text.count("getenv"):
            reads[f] = text.count("getenv")
    assert sorted(reads) == ["comm_ipc.hip", "knobs.hip"] and reads["comm_ipc.hip"] == 1, reads


def both_tables():
    """The rows HPGMG_SWITCHES=1 prints when libhpgmg_fv.so loads: the plugin's switches, then the kernel library's knobs."""
    hip, fv = ensure_built()
    clean = {k: v for k, v in os.environ.items() if not k.startswith("HPGMG_")}
    out = subprocess.run([sys.executable, "-c", "import ctypes, sys; ctypes.CDLL(sys.argv[1], mode=ctypes.RTLD_GLOBAL); ctypes.CDLL(sys.argv[2])", hip, fv],
                         capture_output=True, text=True, timeout=60, env=dict(clean, HPGMG_SWITCHES="1"))
    assert out.returncode == 0, out.stderr[-800:]
    return re.findall(r"^  (HPGMG_\w+) += (-?\d+) +\(default (-?\d+)\)  \S", out.stderr, flags=re.M)


def test_hpgmg_switches_prints_both_tables():
    printed = both_tables()
    names = [n for n, _, _ in printed]
    assert len(names) == len(set(names))
    assert [(n, int(d)) for n, v, d in printed[-len(ROWS):]] == ROWS and all(v == d for _, v, d in printed[-len(ROWS):])
    plugin = names[:-len(ROWS)]      # (the plugin's table has no listing call: its first row, one from its end, and no fewer rows than it had when this was written)
    assert plugin[0] == "HPGMG_GHOST_FREE" and "HPGMG_SMOOTHER_PRECISION" in plugin and len(plugin) >= 32, plugin


# Names of these three families that no library reads: the Python of the tests and of bench.py reads the first group from os.environ to steer a
# worker process; the second group are -D macros of the experiment builds, not environment variables.
NOT_LIBRARY_VARIABLES = {
    "HPGMG_TEST_TRANSPORT", "HPGMG_TEST_FAIL_TRANSPORT", "HPGMG_TEST_BOTTOM_SOLVER", "HPGMG_TEST_UCYCLES", "HPGMG_TEST_CORRUPT_FROM", "HPGMG_TEST_SUBCOMM",
    "HPGMG_TEST_WITH_TORCH",
    "HPGMG_EXP_TIMELINE", "HPGMG_EXP_STATIC_SLOTS",
}


def test_every_knob_named_in_tests_tools_and_documents_is_a_row():
    """A name the libraries would never read is a typo in an A/B script or a stale document.  `HPGMG_TUNE_FV4_*` in a document stands for the rows that begin so."""
    known = set(n for n, _, _ in both_tables())
    files = [os.path.join(ROOT, f) for f in ("bench.py", "README.md", "DESIGN.md", "INTEGRATION.md")]
    for top in ("tests", "tools"):
        for dirpath, dirs, names in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [d for d in dirs if d not in ("golden", "__pycache__")]
            files += [os.path.join(dirpath, n) for n in names if not n.endswith(".pyc")]
    unknown = {}
    for path in files:
        for name in set(re.findall(r"HPGMG_(?:TUNE|TEST|EXP)_[A-Z0-9_]+", open(path, errors="ignore").read())):
            if name in known or name in NOT_LIBRARY_VARIABLES or (name.endswith("_") and any(k.startswith(name) for k in known)):
                continue
            unknown.setdefault(name, []).append(os.path.relpath(path, ROOT))
    assert not unknown, unknown
