"""Differential fuzzing of the HIP path against the oracle (scripts/fuzz_parity.py): random genomes with tandem
repeats, dispersed repeats, inversions, low-complexity runs, N runs, IUPAC codes, lower case, drafts and short contigs,
under random (k, fragment_length, percentage_identity, minimum_fraction).  Every L2 mapping, the index size, the
frequency threshold and every hit must match.  A 10 000-case campaign (seeds 2-5) ran clean in round 1.

The seed is NOT fixed: it is derived from the kernel and oracle sources, so every change of either draws a fresh set of
cases (the same sources always replay the same set; the seed is printed on failure and `scripts/fuzz_parity.py <cases>
<seed>` replays it).  The run is a fixed number of cases -- about 100 s on an idle box -- so that a loaded machine makes the
test slower, not red."""
import hashlib
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def source_seed():
    h = hashlib.sha256()
    for d in ("pyfastani_amd/csrc", "oracle"):
        for name in sorted(os.listdir(os.path.join(ROOT, d))):
            if name.endswith((".h", ".hip", ".hpp", ".cpp")):
                h.update(open(os.path.join(ROOT, d, name), "rb").read())
    return int.from_bytes(h.digest()[:4], "little") & 0x7FFFFFFF


def test_fuzz_against_oracle():
    seed = source_seed()
    cases = 400
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), str(cases), str(seed)],
                         capture_output=True, text=True, timeout=2400)
    assert res.returncode == 0, f"seed {seed}\n" + res.stdout[-3000:] + res.stderr[-3000:]
    assert "0 mismatches" in res.stdout and f"seed {seed}" in res.stdout
    assert int(res.stdout.strip().splitlines()[-1].split()[0]) == cases, res.stdout[-500:]


def test_fuzz_with_the_coordinate_filter_of_large_indices_forced_on():
    """k_l1 skips the coordinate fetch of hits that cannot be an end of a candidate only on indices of 3 x 10^8 records and
    more (where it pays); FA_L1_NEAR=1 forces it onto the small indices of the fuzzer, so that its loci are compared with the
    oracle's mapping for mapping -- chance hits, repeats, tandem duplications, minimum hit counts from 1 up."""
    seed = (source_seed() ^ 0x5A5A5A) & 0x7FFFFFFF
    cases = 250
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), str(cases), str(seed)],
                         env=dict(os.environ, FA_L1_NEAR="1"), capture_output=True, text=True, timeout=2400)
    assert res.returncode == 0, f"seed {seed}\n" + res.stdout[-3000:] + res.stderr[-3000:]
    assert "0 mismatches" in res.stdout and int(res.stdout.strip().splitlines()[-1].split()[0]) == cases, res.stdout[-500:]


def test_fuzz_histories_against_oracle():
    """One index per case, then 4-8 queries on the same mapper -- plain, tandem, drafts, N / IUPAC, batches -- each through a random
    entry point (query_draft, query_genome, GenomeBatch.query(first, count), query_fasta_stream): the sizes and kernel forms one
    query leaves in the mapper's speculation record are what the next one runs with.  Every answer against the oracle."""
    seed = (source_seed() ^ 0x3C3C3C) & 0x7FFFFFFF
    cases = 400
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--history", str(cases), str(seed)],
                         capture_output=True, text=True, timeout=2400)
    assert res.returncode == 0, f"seed {seed}\n" + res.stdout[-3000:] + res.stderr[-3000:]
    assert "0 mismatches" in res.stdout and int(res.stdout.strip().splitlines()[-1].split()[0]) == cases, res.stdout[-500:]


def test_fuzz_window_domain_against_oracle():
    """The ends of the window range (scripts/fuzz_parity.py --domain): identities of 64.5-70 % (w = 2-4, thousands of
    minimizers per fragment) and 96-100 % (sketches of a handful), p-values from 1e-1 to 1e-12, k from 5 to 33."""
    seed = (source_seed() ^ 0x0F0F0F) & 0x7FFFFFFF
    cases = 800
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--domain", str(cases), str(seed)],
                         capture_output=True, text=True, timeout=2400)
    assert res.returncode == 0, f"seed {seed}\n" + res.stdout[-3000:] + res.stderr[-3000:]
    last = res.stdout.strip().splitlines()[-1].split()
    assert "0 mismatches" in res.stdout and int(last[0]) == cases, res.stdout[-500:]
    # (k above ~20 and the lowest identities at small k recommend w = fragment: nothing maps, the case is skipped)
    assert int(last[last.index("degenerate,") - 1]) <= cases * 2 // 3, res.stdout[-500:]


def test_fuzz_contig_domain_against_oracle():
    """Fragmented references and queries (scripts/fuzz_parity.py --contigs): every genome cut into 1-400 contigs at the case's
    own critical lengths (tests/contig_domain.py), half of them with repeats inside their contigs, genomes without a contig
    and genomes of contigs too short for a record.
    A fixed 350 cases: 20.5 s on an MI355X, next to 21.0 s for the --domain leg (800 cases, most of them cheap or degenerate)
    in the same run."""
    seed = (source_seed() ^ 0x717171) & 0x7FFFFFFF
    cases = 350
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--contigs", str(cases), str(seed)],
                         capture_output=True, text=True, timeout=2400)
    assert res.returncode == 0, f"seed {seed}\n" + res.stdout[-3000:] + res.stderr[-3000:]
    last = res.stdout.strip().splitlines()[-1].split()
    assert "0 mismatches" in res.stdout and int(last[0]) == cases, res.stdout[-500:]
    assert int(last[last.index("degenerate,") - 1]) <= cases // 4, res.stdout[-500:]


def test_fuzz_kmer_domain_against_oracle():
    """The k axis (scripts/fuzz_parity.py --kmers): k from the critical list of tests/kmer_domain.py and from 1..64, an explicit
    window out of one per form of K1, genomes by the rules of that module's end-to-end cells.  The oracle mapped something in every one of 1 050 cases of the generator
    on the CPU; a case that maps nothing counts as degenerate, and the bound leaves room for a seed that draws a few.
    A fixed 150 cases: 7.1 s on an MI355X, next to 18.5 s for the --contigs leg (350 cases) in the same run."""
    seed = (source_seed() ^ 0x636363) & 0x7FFFFFFF
    cases = 150
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--kmers", str(cases), str(seed)],
                         capture_output=True, text=True, timeout=2400)
    assert res.returncode == 0, f"seed {seed}\n" + res.stdout[-3000:] + res.stderr[-3000:]
    last = res.stdout.strip().splitlines()[-1].split()
    assert "0 mismatches" in res.stdout and int(last[0]) == cases, res.stdout[-500:]
    assert int(last[last.index("degenerate,") - 1]) <= cases // 20, res.stdout[-500:]


ALL_RULES = "l2_confidence=0.75,slide_end=fragment,cgi_ties=largest"


def test_fuzz_window_domain_under_the_other_readings():
    """The --domain leg with every sketch under the three non-default readings (`--rules`), against the oracle built with the
    matching switches: the longer slide, the other interval and the other tie direction at w = 2-4 and at sketches of a
    handful of records, on genomes with repeats, inversions, N runs and drafts."""
    seed = (source_seed() ^ 0x2B2B2B) & 0x7FFFFFFF
    cases = 200
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--rules", ALL_RULES, "--domain", str(cases), str(seed)],
                         capture_output=True, text=True, timeout=2400)
    assert res.returncode == 0, f"seed {seed}\n" + res.stdout[-3000:] + res.stderr[-3000:]
    last = res.stdout.strip().splitlines()[-1].split()
    assert "0 mismatches" in res.stdout and int(last[0]) == cases and "fragment" in res.stdout.strip().splitlines()[-1], res.stdout[-500:]
    assert int(last[last.index("degenerate,") - 1]) <= cases * 2 // 3, res.stdout[-500:]


def test_fuzz_contig_domain_under_the_other_readings():
    """The --contigs leg under the three non-default readings: loci at contig ends, where the longer slide is clamped, at the
    case's own critical contig lengths."""
    seed = (source_seed() ^ 0x4D4D4D) & 0x7FFFFFFF
    cases = 200
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--rules", ALL_RULES, "--contigs", str(cases), str(seed)],
                         capture_output=True, text=True, timeout=2400)
    assert res.returncode == 0, f"seed {seed}\n" + res.stdout[-3000:] + res.stderr[-3000:]
    last = res.stdout.strip().splitlines()[-1].split()
    assert "0 mismatches" in res.stdout and int(last[0]) == cases and "fragment" in res.stdout.strip().splitlines()[-1], res.stdout[-500:]
    assert int(last[last.index("degenerate,") - 1]) <= cases // 4, res.stdout[-500:]
