"""The host stages of `dicey hunt` on a box without a GPU: dicey_amd/cli/hunt_stages.hpp as a program of its own (plain and under
the host sanitizers), and the one gzip member writer of dicey_amd/cli/cli_common.hpp behind its two callers."""
import os
import re
import struct
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_hunt_stages_program(tmp_path, name, flags):
    """the query reader against the reference's line-by-line loop (19 hand-written files, 2 000 generated ones), the rank plan, the chunk
    packer, the gathered block's size checks and layout, the open-flag truth table"""
    src = os.path.join(ROOT, "tests", "host", "hunt_stages_main.cpp")
    exe = str(tmp_path / ("hunt_stages_" + name))
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, src])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (name, r.stdout, r.stderr)
    assert re.fullmatch(r"ok 2019 files, \d+ records, \d+ joined sequences\n", r.stdout), r.stdout


def test_hunt_stages_header_asks_for_no_library():
    """the header's own includes: the standard library and the plain structs of include/dicey_gpu.h"""
    text = open(os.path.join(ROOT, "dicey_amd", "cli", "hunt_stages.hpp")).read()
    quoted = re.findall(r'#include\s+"([^"]+)"', text)
    assert quoted == ["../../include/dicey_gpu.h"]
    assert not re.search(r"#include\s+<(hip|zlib|rccl)", text)


GZIP_MAIN = r"""
#include "cli_common.hpp"
int main(int, char** argv) {
  std::string buf(100000, '\0'), out;
  uint32_t x = 12345;
  for (char& ch : buf) {
    x = x * 1103515245u + 12345u;
    ch = ((x >> 24) % 61 == 0) ? '\n' : "ACGT"[(x >> 16) & 3];
  }
  if (!gzip_member(buf, out)) return 1;  // mappability's caller: level 1, to a string
  FILE* f = std::fopen(argv[1], "wb");
  if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f) != 0) return 2;
  return append_gzip_member(argv[2], buf) && append_gzip_member(argv[2], std::string()) ? 0 : 3;  // hunt's: default level, appended
}
"""


def _member(data, level):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF]) + z.compress(data) + z.flush() + struct.pack("<II", zlib.crc32(data), len(data))


def test_gzip_members_keep_their_bytes(tmp_path):
    """both callers of the one member writer: the bytes zlib gives at that level under the same header and trailer, and the bytes the
    two separate functions wrote before they were joined (tests/golden/gzip_member_*.gz, written by the parent commit's code)"""
    src = tmp_path / "gzip_main.cpp"
    src.write_text(GZIP_MAIN)
    exe = str(tmp_path / "gzip_main")
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "dicey_amd", "cli"), "-o", exe, str(src), "-lz"])
    one, appended = tmp_path / "level1.gz", tmp_path / "default.gz"
    subprocess.check_call([exe, str(one), str(appended)])
    x, data = 12345, bytearray()
    for _ in range(100000):
        x = (x * 1103515245 + 12345) & 0xFFFFFFFF
        data.append(10 if (x >> 24) % 61 == 0 else b"ACGT"[(x >> 16) & 3])
    data = bytes(data)
    golden = os.path.join(ROOT, "tests", "golden")
    assert one.read_bytes() == _member(data, 1)
    assert one.read_bytes() == open(os.path.join(golden, "gzip_member_level1.gz"), "rb").read()
    assert appended.read_bytes() == _member(data, -1) + _member(b"", -1)
    assert appended.read_bytes()[:-len(_member(b"", -1))] == open(os.path.join(golden, "gzip_member_default.gz"), "rb").read()
    assert zlib.decompress(one.read_bytes(), 31) == data
