#!/usr/bin/env python3
"""Record what the REFERENCE returns on the inputs of the tests that compare against it, so that they run where the
reference is not built: its reader (tests/kseq.h through oracle/ref_kseq_shim.cpp) on the fuzz texts of
test_ingest.py and on its padded gzip files, and its library (oracle/ref_shim.cpp) on the inputs of
test_oracle_golden.py::test_live_against_reference_library, and its reader on the hand-built texts of parse_cases.py
(test_parse_cases.py, test_gpu_parse_cases.py).  Those tests build their inputs with the same
functions used here and still compare live where oracle/_ref exists.
Build container only:  make -C oracle ref && python tests/golden/make_ref_golden.py   -> tests/golden/ref_verdicts.json"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402

if not O.have_ref():
    sys.exit("oracle/_ref/libbiolib_ref.so missing: run `make -C oracle ref` where the reference sources are")

import test_ingest as TI  # noqa: E402
import test_oracle_golden as TO  # noqa: E402
import parse_cases as PC  # noqa: E402
from ingest_fuzz import cases  # noqa: E402

out = {}
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "f.txt")

    def read(data):
        with open(path, "wb") as f:
            f.write(data)
        return TI.reads_verdict(TI._ref_read(path))

    # seeds and counts as the tests draw them (test_fuzz_host_reader_vs_reference_reader, test_fuzz_device_parser_vs_reference_reader)
    for key, seed, n in (("reader_fuzz_host", 11, 600), ("reader_fuzz_device", 12, 400)):
        out[key] = [{"text": hashlib.sha256(t).hexdigest()[:16], "ref": read(t)} for t in cases(seed, n)]
    out["reader_padded_gzip"] = {name: read(data) for name, data in TI.padded_gzip_files()[1].items()}
    # name -> the text's digest and the reader's verdict (past 64 records: the count and a digest of the lengths, parse_cases.compact)
    out["parser_cases"] = {name: {"text": PC.text_sha(t), "ref": PC.compact(read(t))} for name, t in PC.CASES.items()}
out["reference_library"] = TO.library_record(O.ref())

with open(os.path.join(HERE, "ref_verdicts.json"), "w") as f:
    json.dump(out, f, separators=(",", ":"), sort_keys=True)
    f.write("\n")
print("wrote", os.path.join(HERE, "ref_verdicts.json"), os.path.getsize(os.path.join(HERE, "ref_verdicts.json")), "bytes")
