"""K1's 32-bit row key (fithic_amd/csrc/fhx_k1key.hpp) on the host: tests/native/k1_key_check.cpp - a plain program with its own
main that includes the header alone - packs and unpacks every field edge (count -1, 0, 8191, 8192, 2^31 - 1; d 0, 0x3FFFE, 0x3FFFF,
0x40000, 2^31 - 1), inter rows with small and large counts and 10^6 random triples, and fails unless each key either escapes, exactly
when the header's rule says so, or gives back what went in.  Built with -fsanitize=undefined,address it must run clean."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_unpack_round_trip_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "k1_key_check")
    # the sanitizers' runtimes linked into the program (clang does so by itself): nothing has to be loaded in front of it
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"] + static + [
           "-I", os.path.join(ROOT, "fithic_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "k1_key_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("k1_key_check ok:"), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
