"""A plain numpy / Python restatement of what the HiC-Pro converter computes (fithic/utils/HiCPro2FitHiC.py), for the tests:
split() parsing, np.add.at into int64 totals, formatting with str().  test_hicpro_host.py pins it to the real reference's
outputs (tests/golden/hicpro); the GPU tests compare the kernels with it on generated matrices."""
import gzip
import json
import math
import os

import numpy as np

HICPRO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hicpro")


def cases():
    with open(os.path.join(HICPRO, "cases.json")) as f:
        return json.load(f)


CASES = {c["name"]: c for c in cases()} if os.path.exists(os.path.join(HICPRO, "cases.json")) else {}


def fixture_bytes(name):
    with gzip.open(os.path.join(HICPRO, name), "rb") as f:
        return f.read()


def case_inputs(case, tmp_path):
    """the case's input files as plain text under tmp_path (the converter takes no gz input) -> (bed, matrix, bias or None)"""
    out = []
    for kind in ("bed", "matrix", "bias"):
        if case[kind] is None:
            out.append(None)
            continue
        path = os.path.join(str(tmp_path), "%s.%s" % (case["name"], kind))
        with open(path, "wb") as f:
            f.write(fixture_bytes(case[kind]))
        out.append(path)
    return out


def case_outputs(case):
    """the real reference's three decompressed outputs (bias: None when the case has no bias file)"""
    name = case["name"]
    return (fixture_bytes(name + ".contacts.out.gz"), fixture_bytes(name + ".fragments.out.gz"),
            fixture_bytes(name + ".bias.out.gz") if case["bias"] else None)


def text_lines(data):
    """the lines Python's text mode yields for these bytes (\\r\\n and \\r end a line like \\n), without their ends"""
    text = data.decode().replace("\r\n", "\n").replace("\r", "\n")
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return lines


class Model:
    """names: chromosome names in order of first appearance in the bed; frag: index -> (chr id, start text, mid);
    cols: chr1, mid1, chr2, mid2, count (int64, file order); totals: int64 over [index_base, index_base + n_slots)"""

    def __init__(self, bed, matrix, bias=None, res=0):
        self.names, ids, self.frag = [], {}, {}
        for line in text_lines(bed):
            t = line.split()
            if res == 0:
                res = int(t[2]) - int(t[1])
            if t[0] not in ids:
                ids[t[0]] = len(self.names)
                self.names.append(t[0])
            self.frag[int(t[3])] = (ids[t[0]], t[1], int(t[1]) + int(res / 2))
        self.res = res
        self.indices = sorted(self.frag)
        self.index_base = self.indices[0] if self.indices else 0
        self.n_slots = self.indices[-1] - self.index_base + 1 if self.indices else 0
        rows = [line.split() for line in text_lines(matrix)]
        assert all(len(t) == 3 for t in rows)
        i = np.array([int(t[0]) for t in rows], np.int64)
        j = np.array([int(t[1]) for t in rows], np.int64)
        value = [float(t[2]) for t in rows]
        assert all(v == int(v) for v in value)
        count = np.array([int(v) for v in value], np.int64)
        for index in list(i) + list(j):
            if index not in self.frag:
                raise KeyError(int(index))
        self.totals = np.zeros(self.n_slots, np.int64)
        np.add.at(self.totals, i - self.index_base, count)
        np.add.at(self.totals, j - self.index_base, count)
        chr_of = {k: v[0] for k, v in self.frag.items()}
        mid_of = {k: v[2] for k, v in self.frag.items()}
        self.cols = [np.array([chr_of[k] for k in i], np.int64), np.array([mid_of[k] for k in i], np.int64),
                     np.array([chr_of[k] for k in j], np.int64), np.array([mid_of[k] for k in j], np.int64), count]
        self.bias_values = None
        if bias is not None:
            values = [float(line.rstrip()) for line in text_lines(bias)]
            total, n = 0, 0
            for v in values:                                         # left to right: the reference's rounding order
                if not math.isnan(v):
                    total += v
                    n += 1
            avg = total / n
            self.bias_values = [-1 if math.isnan(v) else v / avg for v in values]

    def contacts_text(self):
        c1, m1, c2, m2, n = self.cols
        return "".join(self.names[c1[r]] + "\t" + str(m1[r]) + "\t" + self.names[c2[r]] + "\t" + str(m2[r]) + "\t" + str(n[r]) + "\n"
                       for r in range(len(n)))

    def fragments_text(self):
        out = []
        for index in self.indices:
            c, start, mid = self.frag[index]
            tcc = int(self.totals[index - self.index_base])
            out.append(self.names[c] + "\t" + start + "\t" + str(mid) + "\t" + str(tcc) + "\t" + str(1 if tcc > 0 else 0) + "\n")
        return "".join(out)

    def bias_text(self):
        out = []
        for k, v in enumerate(self.bias_values):
            c, _, mid = self.frag[k + 1]
            out.append(self.names[c] + "\t" + str(mid) + "\t" + str(v) + "\n")
        return "".join(out)
