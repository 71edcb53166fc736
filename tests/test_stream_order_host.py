"""The table of test_stream_order_gpu.py held against include/fdr.h, on the CPU: it names exactly the entry points that take a
`void* stream`, every exemption from "does not wait" quotes the header, and the Python wrappers it goes through exist and take
`stream=`.  An entry added to fdr.h without a fenced case fails here."""
import inspect
import os
import re

from test_stream_order_gpu import CASES, ENTRIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "fdr.h")) as f:
        return f.read()


def _plain(text):
    """the header as running text: comment marks and the ` *` line starts out, whitespace collapsed"""
    text = text.replace("/*", " ").replace("*/", " ")
    text = re.sub(r"(?m)^\s*\*(?=\s|$)", " ", text)
    return re.sub(r"\s+", " ", text)


def stream_entries(text):
    """the functions declared in fdr.h with a `void* stream` parameter"""
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = set()
    for m in re.finditer(r"\bint\s+(fdr_\w+)\s*\(([^;{]*)\)\s*;", code):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            found.add(m.group(1))
    return found


def test_the_parser_reads_declarations_of_every_shape():
    text = """/* int fdr_in_a_comment(void* stream); */
    int fdr_one(int device, float* d_out, void* stream);
    int fdr_two(fdr_plan* plan, const float* d_img,
                int rows, void *stream);
    int fdr_host_form(fdr_plan* plan, const float* img_host);
    int fdr_other_pointer(void* d_dst, size_t bytes);"""
    assert stream_entries(text) == {"fdr_one", "fdr_two"}
    assert _plain("/* a\n *    b  c\n * d */") .strip() == "a b c d"


def test_every_entry_with_a_stream_has_a_fenced_case():
    declared = stream_entries(_header())
    assert len(declared) >= 60, "the parser lost the declarations: %d found" % len(declared)
    assert declared - ENTRIES == set(), "entry points with a stream parameter and no fenced case: %s" % sorted(declared - ENTRIES)
    assert ENTRIES - declared == set(), "the table names entries fdr.h does not declare with a stream: %s" % sorted(ENTRIES - declared)


def test_every_exemption_quotes_the_header():
    plain = _plain(_header())
    exempt = [c for c in CASES if c.exempt is not None]
    assert exempt, "the table lost its exemptions"
    for c in exempt:
        assert len(c.exempt) >= 40, "%s: an exemption must be a sentence, not a word: %r" % (c.id, c.exempt)
        assert re.sub(r"\s+", " ", c.exempt) in plain, "%s: the exemption does not occur in include/fdr.h: %r" % (c.id, c.exempt)


def test_the_wrappers_exist_and_take_a_stream(fdr):
    for c in CASES:
        for name in c.wrappers:
            obj = fdr
            for part in name.split("."):
                assert hasattr(obj, part), "%s: no %s in the package" % (c.id, name)
                obj = getattr(obj, part)
            assert "stream" in inspect.signature(obj).parameters, "%s: %s takes no stream=" % (c.id, name)
        for entry in c.entries:
            assert entry in fdr.EXPORTED_SYMBOLS and hasattr(fdr.lib, entry), "%s: libfdr.so does not export %s" % (c.id, entry)


def test_the_table_keeps_the_cases_the_design_names():
    ids = {c.id for c in CASES}
    for must in ("wiener-simple", "wiener-parity", "wiener-fast-full", "wiener-fast-half", "wiener-mixed", "wiener-any-size", "wiener-long-rows",
                 "wiener-batch-fast-half-streams", "wiener-batch-graph-replay", "wiener-batch-graph-capture", "tiled-rl", "tiled-tv",
                 "rl-auto-none", "tv-auto", "batch-tv-auto", "frames-rl", "blind-free-weights"):
        assert must in ids, must
