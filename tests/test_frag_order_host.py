"""The one-genome workgroup order of k_l2_events as arithmetic (csrc/fa_policy.h: one_genome_run, one_genome_frag), no GPU:
scripts/host_sanitize/frag_order.cpp under AddressSanitizer + UBSan -- for every fragment count from the gate to 4096 the closed
form visits every fragment once, gives every other workgroup -1, and equals the table of build_frag_order entry by entry."""
import os
import subprocess

from conftest import ROOT


def test_closed_form_against_the_table_under_sanitizers():
    out = os.path.join(ROOT, "build", "host_sanitize")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "frag_order_pytest")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "host_sanitize", "frag_order.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "all checks passed" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    # 2 tables of 8 * ceil(F / 8) entries for every F in 64 .. 4096
    assert f"({2 * sum(8 * ((F + 7) // 8) for F in range(64, 4097))} table entries)" in res.stdout, res.stdout
