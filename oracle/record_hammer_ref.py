"""Records tests/golden/hammer_ref/ from the reference's own BayesHammer code: `python -m oracle.record_hammer_ref`.

TEST INFRASTRUCTURE ONLY.  Runs oracle/_ref/hammer_ref (built by `make -C oracle ref` from the reference's sources and
oracle/hammer_ref_driver.cpp) on the inputs of tests/hammer_ref_case.py and stores every stage's dump as
<case>_<stage>.json.gz with a `_provenance` entry.  Recording twice gives the same bytes (gzip without a time stamp,
sorted keys), which is what the drift guard of tests/test_hammer_reference_fixtures.py relies on.
"""
import gzip
import io
import json
import os
import subprocess
import sys
import tempfile

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
BINARY = os.path.join(_HERE, "_ref", "hammer_ref")
CONFIG = os.path.join(_ROOT, "tests", "golden", "hammer_config.info")
THREADS = dict(general_max_nthreads=1, count_merge_nthreads=1, bayes_nthreads=1, expand_nthreads=1, correct_nthreads=1,
               omp_set_num_threads=1)
OVERRIDES = dict(count_filter_singletons=0, general_tau=1, general_max_iterations=1, general_debug=0, K=21)


def _config_values():
    out = {}
    for line in open(CONFIG):
        f = line.split(";")[0].split()
        if f:
            out[f[0]] = f[1] if len(f) > 1 else ""
    for key in ("dataset", "input_working_dir", "output_dir"):  # set per run
        out.pop(key)
    out.update({k: str(v) for k, v in OVERRIDES.items() if k != "K"})
    out.update({k: "1" for k in THREADS if k != "omp_set_num_threads"})
    return out


def _rows(path):
    with open(path, encoding="latin-1") as f:
        return [line.rstrip("\n").split("\t") for line in f if not line.startswith("#")]


def _list(field, conv):
    return [] if field == "-" else [conv(x) for x in field.split(",")]


def run_driver(case, tmp):
    """runs the reference on a case in `tmp`; returns {stage: data}"""
    from tests import hammer_ref_case as C
    left, right, names = C.case_texts(case)
    d = os.path.join(tmp, case)
    dirs = {x: os.path.join(d, x) for x in ("in", "work", "out", "dump")}
    for x in dirs.values():
        os.makedirs(x)
    paths = [os.path.join(dirs["in"], n) for n in names]
    for p, text in zip(paths, (left, right)):
        with open(p, "w", encoding="latin-1") as f:
            f.write(text)
    r = subprocess.run([BINARY, CONFIG, paths[0], paths[1], dirs["work"], dirs["out"], dirs["dump"]],
                       capture_output=True, text=True, errors="replace")
    if r.returncode != 0:
        raise RuntimeError("hammer_ref failed on %s (%d):\n%s\n%s" % (case, r.returncode, r.stdout[-3000:], r.stderr[-3000:]))
    dump = dirs["dump"]
    prov = dict(command="oracle/_ref/hammer_ref tests/golden/hammer_config.info %s %s <work> <out> <dump>" % names,
                recorder="python -m oracle.record_hammer_ref", threads=THREADS, overrides=OVERRIDES,
                config=_config_values(), input_md5={names[0]: C.md5(left), names[1]: C.md5(right)})
    st = {}
    reads = []
    for f in _rows(os.path.join(dump, "stage0.tsv")):
        s2, p2, s4, p4 = _list(f[6], int), _list(f[7], float), _list(f[8], int), _list(f[9], float)
        at2 = dict(zip(s2, p2))
        # threshold 4 as its difference from threshold 2: the probabilities are equal wherever the walk is the same
        reads.append(dict(file=int(f[0]), name=f[1], ltrim=int(f[2]), rtrim=int(f[3]), initial_size=int(f[4]), size=int(f[5]),
                          starts_q2=s2, probs_q2=p2, starts_q4=s4,
                          probs_q4_where_not_q2=[[s, p] for s, p in zip(s4, p4) if at2.get(s) != p]))
    st["stage0"] = dict(
        reads=reads,
        printed=[open(os.path.join(dump, "stage0_print_%d.fastq" % i), encoding="latin-1").read() for i in (1, 2)])
    rows = _rows(os.path.join(dump, "stage1.tsv"))
    st["stage1"] = dict(kmers=[f[0] for f in rows], count=[int(f[1]) for f in rows], total_qual=[f[2] for f in rows],
                        total_qual_bits=[f[3] for f in rows], qual_words=[[f[4], f[5]] for f in rows])
    st["stage2"] = dict(clusters=[line.split() for line in open(os.path.join(dump, "stage2.tsv")).read().split("\n") if line])
    rows = _rows(os.path.join(dump, "stage3.tsv"))
    st["stage3"] = dict(kmers=[f[0] for f in rows], good="".join(f[1] for f in rows), count=[int(f[2]) for f in rows],
                        new_centres=[f[0] for f in rows if f[3] == "1"])
    rows = _rows(os.path.join(dump, "stage4.tsv"))
    extra = _rows(os.path.join(dump, "stage4_extra.tsv"))
    st["stage4"] = dict(rounds=[dict(round=int(f[0]), added=int(f[1]), good=f[2]) for f in rows], extra_pass_added=int(extra[0][1]))
    files = _rows(os.path.join(dump, "stage5_files.tsv"))
    st["stage5"] = dict(dataset=[[f[0], f[1]] for f in files if f[0] != "changed_reads"],
                        changed_reads=int([f[1] for f in files if f[0] == "changed_reads"][0]),
                        files={n: open(os.path.join(dirs["out"], n), encoding="latin-1").read()
                               for n in sorted(os.listdir(dirs["out"])) if n.endswith(".fastq")},
                        log=[line for line in r.stdout.split("\n") if "Correction done" in line or "Failed to correct" in line])
    for v in st.values():
        v["_provenance"] = prov
    return st


def encode(data):
    """the bytes of a fixture file: canonical JSON, gzip with no time stamp and no file name"""
    raw = json.dumps(data, sort_keys=True, separators=(",", ":")).encode("latin-1")
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, mtime=0, compresslevel=9) as f:
        f.write(raw)
    return buf.getvalue()


def record(tmp):
    """{file name: bytes} of every fixture"""
    from tests import hammer_ref_case as C
    out = {}
    for case in C.CASES:
        for stage, data in run_driver(case, tmp).items():
            if stage == "stage0":  # one file per side: the probabilities do not compress
                for side in (0, 1):
                    part = dict(reads=[r for r in data["reads"] if r["file"] == side], printed=data["printed"][side],
                                _provenance=data["_provenance"])
                    out["%s_stage0_%d.json.gz" % (case, side + 1)] = encode(part)
                continue
            out["%s_%s.json.gz" % (case, stage)] = encode(data)
    return out


def main():
    from tests import hammer_ref_case as C
    if not os.path.exists(BINARY):
        sys.exit("oracle/_ref/hammer_ref is not built: run `make -C oracle ref` with the reference tree present")
    os.makedirs(C.FIXTURES, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, data in sorted(record(tmp).items()):
            with open(os.path.join(C.FIXTURES, name), "wb") as f:
                f.write(data)
            print("%-28s %7d bytes" % (name, len(data)))


if __name__ == "__main__":
    sys.path.insert(0, _ROOT)
    main()
