#!/usr/bin/env python3
"""profiles/bgzf_deflate_sizes.txt: the size of the BGZF member the device's deflater (k_bgzf_block) writes for every block of the cases
of tests/test_bgzf_deflate.py, next to zlib's for the same block with Z_RLE (runs at distance 1 only: the device's kind of match) and
Z_HUFFMAN_ONLY (no matches), level 6, each plus the 26 bytes of BGZF framing.  Needs the GPU.  usage: tools/bgzf_deflate_sizes.py [out]"""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deflate_spec as ds                     # noqa: E402
import test_bgzf_deflate as t                 # noqa: E402
from bitmapperbs_amd import mapper            # noqa: E402


def zsize(block, strategy):
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, strategy)
    return len(co.compress(block) + co.flush()) + 26


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bgzf_deflate_sizes.txt")
    cases = [("a uniform", t.gen_uniform(1, t.BLK))]
    cases += [("b %d values" % k, t.gen_uniform(k, t.BLK, k)) for k in (250, 252, 254)]
    cases += [("c skewed, no run", t.gen_skewed(2, t.BLK)), ("d one value", b"\xa7" * t.BLK), ("e run sweep", t.gen_runs()[0]),
              ("f period 2", b"AB" * (t.BLK // 2)), ("f period 3", b"ABC" * (t.BLK // 3)), ("g deep", t.gen_deep(3, False)),
              ("g deep + bush", t.gen_deep(3, True)), ("h every symbol", t.gen_all_symbols(4))]
    cases += [("k fuzz %d" % s, b"".join(t.gen_fuzz(s))) for s in range(100, 110)]
    m = mapper.Mapper(None, 0)
    lines = ["# device BGZF member sizes (bytes, header and trailer included) against zlib level 6 on the same block",
             "# written by tools/bgzf_deflate_sizes.py; dev/huff = device size / Z_HUFFMAN_ONLY size",
             "%-18s %5s %6s %5s %7s %7s %7s %8s" % ("case", "block", "input", "BTYPE", "device", "Z_RLE", "Z_HUFF", "dev/huff")]
    for name, chosen in cases:
        stream, lens = t.framed(chosen)
        mem = ds.members(m.bam_sort(stream, lens))[1:]
        for i, x in enumerate(mem):
            block = chosen[i * t.BLK:(i + 1) * t.BLK]
            assert zlib.decompress(x["payload"], -15) == block
            h = zsize(block, zlib.Z_HUFFMAN_ONLY)
            lines.append("%-18s %5d %6d %5d %7d %7d %7d %8.3f" % (name, i, len(block), (x["payload"][0] >> 1) & 3, x["bsize"], zsize(block, zlib.Z_RLE), h, x["bsize"] / h))
    m.close()
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
