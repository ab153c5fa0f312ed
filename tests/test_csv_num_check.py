"""The CSV reader's number conversion on a CPU: builds tools/csv_num_check.cpp
with csrc/knn_csv_num.h alone (g++, AddressSanitizer and UBSan where their
runtimes are installed) and runs it as a child process.  The program converts
the tricky tokens, the boundary cases and over two million generated tokens
with csv_fast_atof / csv_fast_atoi, compares every converted token with atof /
atoi bit for bit, and exits non-zero on a mismatch, on a slow token among the
tier 1 generators or on more than 1 % slow tokens among %.17g normals."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "-mpi-knn-_amd")


def test_every_converted_token_carries_atofs_bits():
    built = subprocess.run(["make", "-s", "-C", PKG, "bin/csv_num_check"], capture_output=True,
                           text=True)
    if built.returncode != 0:  # no sanitizer runtimes on this machine: the plain program
        built = subprocess.run(["make", "-s", "-C", PKG, "bin/csv_num_check", "SAN="],
                               capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    run = subprocess.run([os.path.join(PKG, "bin", "csv_num_check")], capture_output=True,
                         text=True)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-4000:] + run.stderr[-4000:])
    assert "\n0 mismatches" in run.stdout


def test_header_compiles_without_a_device_toolchain(tmp_path):
    """knn_csv_num.h with plain g++ and no ROCm include path."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "knn_csv_num.h"\nint main() { return 0; }\n')
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I",
                          os.path.join(PKG, "csrc"), "-c", str(src), "-o",
                          str(tmp_path / "t.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
