"""CPU-only: tests/cpp/lz4f_dict_encode_asan_main.cpp -- the emulator unit of the frame encode with a dictionary as a stand-alone
program with a main of its own -- compiled with g++ under AddressSanitizer and UBSan and run as a program.  Nothing loaded into Python
is sanitized."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_sequences_under_address_sanitizer(tmp_path):
    exe = str(tmp_path / "lz4f_dict_encode_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-pthread",
                    "-Wno-unknown-pragmas",
                    "-I" + os.path.join(ROOT, "tests", "simt"), "-I" + os.path.join(ROOT, "lz4net_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "lz4f_dict_encode_asan_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "20 cases ok" in run.stdout
