"""The knob table of the library (csrc/fa_knobs.h), no GPU: its parsers and read times under AddressSanitizer + UBSan
(scripts/host_sanitize/knobs.cpp), and its names against the sources, the README's table and every FA_* name the tests and
scripts set -- a knob exists where the table has a row, and nowhere else."""
import glob
import os
import re
import subprocess

from conftest import ROOT
from pyfastani_amd import _batch

CSRC = os.path.join(ROOT, "pyfastani_amd", "csrc")
ROW = re.compile(r'^\s*X\((\w+),\s*"(FA_[A-Z0-9_]+)",\s*(FLAG|NUM|COUNT|COUNT_IN\([^)]*\)|COUNT_UP\([^)]*\)|TEXT),\s*([^,]+),\s*(ONCE|LIVE),\s*"([^"]+)"\)', re.M)
# FA_* names that are no knob of the library: variables of the Python layer, of bench.py and of the scripts, error codes and macros
NOT_KNOBS = {"FA_FORCE_DIST", "FA_ORACLE_DEFINES", "FA_HEAD", "FA_OK", "FA_KW_CELLS", "FA_EV_WAVES", "FA_EV_RPL",
             "FA_TIMING_SLOTS", "FA_SPEC_FIELDS"}            # (the last two: the tables of csrc/fa_diag.h)
NOT_KNOB_PREFIXES = ("FA_BENCH", "FA_PROFILE_", "FA_ERR_")


def table():
    """{name: (identifier, kind, default, when)} of the header's table."""
    with open(os.path.join(CSRC, "fa_knobs.h")) as f:
        rows = ROW.findall(f.read())
    assert len(rows) == len({r[1] for r in rows}) == len({r[0] for r in rows}) >= 30, rows
    return {name: (ident, kind, dflt.strip(), when) for ident, name, kind, dflt, when, _ in rows}


def readme_rows():
    with open(os.path.join(ROOT, "README.md")) as f:
        return [line for line in f if line.startswith("| `FA_")]


def test_parsers_and_read_times_under_sanitizers():
    """scripts/host_sanitize/knobs.cpp: the strings of every kind against values written out by hand, ONCE against LIVE, and
    every default -- two runs, since a ONCE accessor answers one question per process."""
    out = os.path.join(ROOT, "build", "host_sanitize")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "knobs_pytest")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "host_sanitize", "knobs.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    for mode in ([], ["defaults"]):
        res = subprocess.run([exe] + mode, capture_output=True, text=True, timeout=300, env=dict(os.environ, FA_TRACE="1", FA_SPIN_US="7"))
        assert res.returncode == 0 and "all checks passed" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
        assert f"{len(table())} knobs" in res.stdout, res.stdout


def test_the_table_is_the_only_reader_of_the_environment():
    reads = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(path) == "fa_knobs.h":
            continue
        with open(path) as f:
            reads += [(os.path.basename(path), line.strip()) for line in f if "getenv(" in line]
    assert [r for r in reads if 'getenv("LOCAL_WORLD_SIZE")' not in r[1]] == [], reads
    assert len(reads) == 1, reads
    # and nothing names a knob behind the table's back: a name string of a knob appears in the table alone
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(path) != "fa_knobs.h":
            with open(path) as f:
                assert not re.findall(r'"FA_[A-Z0-9_]+"', f.read()), path


def test_every_name_in_use_is_in_the_table():
    names = set(table())
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "scripts", "*.py")) + glob.glob(os.path.join(ROOT, "scripts", "*.sh"))
    assert len(files) > 60
    unknown = {}
    texts = {path: open(path).read() for path in files}
    texts["README.md (the table)"] = "".join(readme_rows())
    for path, text in texts.items():
        for tok in set(re.findall(r"\bFA_[A-Z0-9_]+", text)):
            if tok not in names and tok not in NOT_KNOBS and not tok.startswith(NOT_KNOB_PREFIXES):
                unknown.setdefault(tok, []).append(os.path.relpath(path, ROOT) if os.path.isabs(path) else path)
    assert not unknown, unknown


def test_readme_table_and_header_table_hold_the_same_names():
    rows = readme_rows()
    listed = [re.match(r"\| `(FA_[A-Z0-9_]+)` \|", line).group(1) for line in rows]
    assert len(listed) == len(set(listed)), listed
    assert set(listed) == set(table()), set(listed) ^ set(table())
    assert all(line.count("|") >= 5 for line in rows)          # name, default, when read, what it does
    # "once" in the README where the header says ONCE, and only there
    when = {name: row[3] for name, row in table().items()}
    for name, line in zip(listed, rows):
        assert line.split("|")[3].strip().startswith("once") == (when[name] == "ONCE"), line


def test_python_default_of_pass_fragments_is_the_headers(monkeypatch):
    monkeypatch.delenv("FA_PASS_FRAGMENTS", raising=False)
    ident, kind, dflt, when = table()["FA_PASS_FRAGMENTS"]
    assert (kind, when) == ("COUNT", "ONCE") and re.fullmatch(r"[0-9 *]+", dflt), (kind, dflt, when)
    assert _batch.pass_fragments() == eval(dflt) == 49152
