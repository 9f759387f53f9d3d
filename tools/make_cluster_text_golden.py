"""Write tests/golden/cluster_text_edge.npz: the reference's own ``parse_file`` on hand-written cluster files that hold every edge case of the
device parser's contract (csrc/cluster_text.hip).

    python tools/make_cluster_text_golden.py --reference <the reference's root directory>

``build_node_dict`` and ``parse_file`` of the reference's ``Code/process.py`` run here in-process, neither restated, through
``tests/golden/make_golden.py::ref_functions`` (the way ``g9_process`` runs them).  Every case is one small file and one ``max_cluster_size``.
The fixture stores, per case, only the text (uint8), the bound, and either what the reference returned (``len_<case>`` / ``flat_<case>``) or the
name of the exception class it raised (``exc_<case>``) with the byte offset of the item that is the first to offend (``off_<case>``, known here
because the text is assembled from pieces).  It stores no program text.

The genome: chr1 (12.3 Mb), chr10 (8 Mb), chr1_random (2.5 Mb) and chrX (5 500 001 b) at 1 Mb; chrY is in the size file but not listed.
"""
import argparse
import io
import os
import shutil
import sys
import tempfile
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 1000000
CHROM_LIST = ["chr1", "chr10", "chr1_random", "chrX"]
SIZES = [("chr1", 9000000), ("chr1", 12300000), ("chr10", 8000000), ("chr1_random", 2500000), ("chrY", 3000000), ("chrX", 5500001)]


def line(*items, cid=b"c"):
    return b"\t".join([cid] + [i if isinstance(i, bytes) else i.encode() for i in items])


def accepted_cases():
    """name -> (text, max_cluster_size)"""
    c = {}
    a, b, d = "chr1:5", "chr1:1500000", "chr1:2500000"
    # rule 1: every way a line can end; the last line has no terminator
    c["newlines"] = (line(a, b) + b"\n" + line(a, d) + b"\r\n" + line(b, d) + b"\r" + line(a, "chr10:0") + b"\n\n\r\r\n" + line(b, "chrX:5500000"), 6)
    c["only_terminators"] = (b"\n\r\n\r\r\n", 6)
    c["empty"] = (b"", 6)
    c["no_final_newline"] = (line(a, b, d), 6)
    # rule 2: strip before split -- leading tabs eat the first item as the "id"; trailing tabs add nothing; every byte str.strip() removes
    c["leading_tabs"] = (b"\t" + b"\t".join([a.encode(), b.encode(), d.encode()]) + b"\n" + b"\t\t" + line(a, b, cid=b"chr1:7") + b"\n", 6)
    c["trailing_tabs"] = (line(a, b) + b"\t\t\t\n" + line(a, d) + b"\t \t\n", 6)
    c["strip_set"] = (b" \x0b\x0c\x1c\x1d\x1e\x1f" + line(a, b) + b"\x1f\x1e\x1d\x1c\x0c\x0b \n" + b"  " + line(b, d) + b"  \r\n" +
                      b"\x1c" + line(a, d, cid=b"id with\x0bblanks") + b"\x0c\n", 6)
    c["blank_lines"] = (b"   \n\t\t\t\n \t \n" + line(a, b) + b"\n\x0b\n", 6)
    # rule 3: the pre-filter counts unparsed items
    c["prefilter_over"] = (line(*([a, b] * 50 + [a])) + b"\n" + line(a, b) + b"\n", 2)                  # 101 items at max 2: skipped, though 2 nodes
    c["prefilter_exact"] = (line(*([a, b] * 50)) + b"\n" + line(b, d) + b"\n", 2)                       # exactly 100 items: parsed, 2 nodes, kept
    c["prefilter_malformed"] = (line("chr1") + b"\n" + line(*(["::", "chr1:x", ""] * 34)) + b"\n" + line("") + b"\n" + line(a, b) + b"\n", 2)
    c["single_item"] = (line(a) + b"\n" + b"justanid\n" + line(a, b) + b"\n", 6)
    # rule 4: names compare exactly; unlisted names drop the item before its position is read; leading zeros; first and last bins
    c["name_prefixes"] = (line("chr1:0", "chr10:0", "chr1_random:0", "chrX:0") + b"\n" + line("chr1_rando:0", "chr1_random:999999", "chr1_random:1000000") + b"\n" +
                          line("chr:5", "chr100:5", "chr1 :5", "Chr1:5", "chr1:1000000", "chr10:1000000") + b"\n", 6)
    c["unlisted_dropped"] = (line("chrZ:xx", a, "chrY:5", b, "chrY:", "chrZ:-1", "chrY:99999999999999999999") + b"\n" + line("chrY:1", "chrY:2000000", a) + b"\n", 6)
    c["leading_zeros"] = (line("chr1:0001500000", "chr1:000000000000000005", "chr10:00") + b"\n", 6)
    c["last_bins"] = (line("chr1:13999999", "chr1:13000000", "chr1:12999999", "chr10:8999999", "chr1_random:3999999", "chrX:6999999", "chrX:0") + b"\n", 10)
    # rule 5: duplicates collapse, ids ascend, the size filter, file order
    c["duplicates"] = (line(d, a, b, a, d, "chr1:2999999", "chr1:1") + b"\n" + line("chrX:5", "chr1:5", "chr10:5", "chr1_random:5") + b"\n", 6)
    c["size_filter"] = (line(*["chr1:%d" % (i * RES) for i in range(7)]) + b"\n" + line(*["chr1:%d" % (i * RES) for i in range(6)]) + b"\n" +
                        line(a, "chr1:999999") + b"\n" + line(a, "chrY:5") + b"\n" + line(b, d) + b"\n", 6)
    c["file_order"] = (b"".join(line("chr1:%d" % ((13 - i) * RES), "chr10:%d" % ((i % 9) * RES), cid=b"k%d" % i) + b"\n" for i in range(14)), 6)
    return c


def error_cases():
    """name -> (the text in front of the offending item, the item, the text behind it, max_cluster_size)"""
    a, b = "chr1:5", "chr1:1500000"
    good = line(a, b) + b"\n"
    e = {}
    e["empty_item"] = (good + b"c\t" + a.encode() + b"\t", b"", b"\t" + b.encode() + b"\n", 6)
    e["no_colon"] = (good + b"c\t" + a.encode() + b"\t", b"chr10", b"\n", 6)
    e["no_colon_unlisted"] = (good + b"c\t" + a.encode() + b"\t", b"chrZ", b"\t" + b.encode() + b"\n", 6)
    e["two_colons"] = (b"c\t", b"chr1:5:6", b"\t" + b.encode() + b"\n" + good, 6)
    e["two_colons_unlisted"] = (good + good + b"c\t" + b.encode() + b"\t", b"chrY:5:", b"\r\n", 6)
    e["bin_past_end"] = (good + b"c\t" + a.encode() + b"\t", b"chr1:14000000", b"\n", 6)
    e["bin_past_end_short_chrom"] = (b"c\t" + a.encode() + b"\t", b"chr1_random:4000000", b"\t" + b.encode(), 6)
    e["bin_far_past_end"] = (b"c\t", b"chrX:999999999999999999", b"\t" + b.encode() + b"\n", 6)
    e["not_a_number"] = (good + b"c\t", b"chr1:x", b"\t" + b.encode() + b"\n", 6)
    e["empty_position"] = (good + b"c\t" + a.encode() + b"\t", b"chr10:", b"\n", 6)
    e["letters_after_digits"] = (b"c\t" + a.encode() + b"\t", b"chr1:15e5", b"\n", 6)
    # two offending items of different classes: the first in the file is the one that is raised
    e["first_of_two_a"] = (good + b"c\t", b"chr1:x", b"\tchr10\n" + b"c\tchr1:99000000\t" + a.encode() + b"\n", 6)
    e["first_of_two_b"] = (good + b"c\t", b"chr1:99000000", b"\tchr1:x\n" + b"c\tchr1\t" + a.encode() + b"\n", 6)
    e["first_of_two_c"] = (b"skipped\tchr1:x\n" + good + b"c\t", b"chr1", b"\tchr1:x\tchr1:99000000\n", 6)
    # an offending item behind a line the pre-filter skips, and on a line of exactly 50 max items
    e["behind_skipped_lines"] = (line(*["::"] * 101) + b"\n" + line("::") + b"\n" + b"c\t" + a.encode() + b"\t", b"::", b"\n", 2)
    e["on_a_line_of_50_max"] = (b"c\t" + b"\t".join([a.encode()] * 99) + b"\t", b"chr1", b"\n", 2)
    return e


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="the reference's root (holds Code/process.py)")
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "cluster_text_edge.npz"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import math
    import pandas as pd
    from tests.golden import make_golden as MG
    MG.REF = os.path.join(args.reference, "Code")

    tmp = tempfile.mkdtemp(prefix="matcha_cluster_text_")
    size_text = "".join("%s\t%d\n" % kv for kv in SIZES)
    with open(os.path.join(tmp, "sizes.txt"), "w") as f:
        f.write(size_text)
    path = os.path.join(tmp, "x.cluster")
    glb = dict(np=MG._NpProxy(), pd=pd, math=math, os=os, sys=sys, tqdm=lambda x: x, trange=range, print=lambda *a, **k: None,
               chrom_size=os.path.join(tmp, "sizes.txt"), chrom_list=CHROM_LIST, res=RES, temp_dir=tmp, cluster_path=path, max_cluster_size=6)
    MG.ref_functions("process.py", {"build_node_dict", "parse_file"}, glb)
    with redirect_stdout(io.StringIO()):
        glb["build_node_dict"]()

    def reference(text, max_size):
        with open(path, "wb") as f:
            f.write(text)
        glb["max_cluster_size"] = max_size
        with redirect_stdout(io.StringIO()):
            glb["parse_file"]()
        return [list(e) for e in np.load(os.path.join(tmp, "edge_list.npy"), allow_pickle=True)]

    out = {"sizes_text": np.array(size_text), "chrom_list": np.array(CHROM_LIST), "res": np.int64(RES),
           "chrom_range": np.load(os.path.join(tmp, "chrom_range.npy"))}
    names, total = [], 0
    for name, (text, max_size) in accepted_cases().items():
        edges = reference(text, max_size)
        out["text_" + name] = np.frombuffer(text, dtype=np.uint8)
        out["max_" + name] = np.int64(max_size)
        out["len_" + name] = np.array([len(e) for e in edges], dtype=np.int64)
        out["flat_" + name] = np.array([v for e in edges for v in e], dtype=np.int64)
        names.append(name)
        total += len(text)
        print("%-22s %6d bytes -> %d clusters" % (name, len(text), len(edges)))
    out["accepted"] = np.array(names)
    names = []
    for name, (front, item, back, max_size) in error_cases().items():
        text = front + item + back
        try:
            reference(text, max_size)
        except Exception as exc:                                               # the class is what the fixture records
            out["exc_" + name] = np.array(type(exc).__name__)
        else:
            raise SystemExit("%s: the reference raised nothing" % name)
        out["text_" + name] = np.frombuffer(text, dtype=np.uint8)
        out["max_" + name] = np.int64(max_size)
        out["off_" + name] = np.int64(len(front))
        names.append(name)
        total += len(text)
        print("%-22s %6d bytes -> %s at byte %d" % (name, len(text), out["exc_" + name], len(front)))
    out["errors"] = np.array(names)
    assert total < 100000
    np.savez_compressed(args.out, **out)
    shutil.rmtree(tmp)
    print("%s: %d bytes of text, %d bytes" % (args.out, total, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
