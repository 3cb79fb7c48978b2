"""csrc/srs_file.hpp, the framing of an SRS file behind kh_srs_write_file and kh_srs_create_from_file, on the host alone: tests/cpp/test_srs_file.cpp
round-trips small files and walks every truncation length, every marker and the count, over heap blocks of exactly the length the reader is told.
Built with g++ under AddressSanitizer and UBSan here -- host code only, no GPU, no library, nothing preloaded."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_framing_reader_and_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_srs_file")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_srs_file.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0 and "srs_file OK" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])
