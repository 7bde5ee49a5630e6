"""oracle/extract_ref.py, the cutter of the reference's hot-path functions, on synthetic text (CPU,
no reference needed): it finds a definition by name whatever precedes it, takes it whole and
unmodified, and refuses a name that is missing or defined twice."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("extract_ref", os.path.join(REPO, "oracle", "extract_ref.py"))
E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E)

SRC = '''#include "x.h"
using namespace std;
// void f(int a) { commented out }
EXPORT void f(int a);            /* a prototype */
#if defined ALL || defined F
#undef F
/** doc { */
EXPORT void
f(int a) {
#ifndef __AVX2__
    for (int j = 0; j < a; ++j) g("}{");
#else
    { __asm__ ("jb 0b\\n" : "=r"(a) : "0"(a) : "memory"); }
#endif
}
#endif
void f_16(int a) { f(a); }
K::K(const P* p, int n): p(p),
    n(n) {}
K::~K() {}
__global__ void kern(int *d) { int id = blockIdx.x; if (id < 1) { d[id] = 0; } }
'''


def _write(tmp_path, text):
    (tmp_path / "a.cu").write_text(text)
    return str(tmp_path)


def test_cuts_the_definition_whole_and_unmodified(tmp_path):
    d = _write(tmp_path, SRC)
    got = E.cut(d, "a.cu", "f")
    body = got.split("\n", 2)[2]
    assert got.startswith("\n// ---- a.cu:8-15\n")
    assert body == SRC[SRC.index("EXPORT void\nf(int a) {"):SRC.index("#endif\nvoid f_16")]
    assert E.cut(d, "a.cu", "f_16").split("\n", 2)[2] == "void f_16(int a) { f(a); }\n"
    assert E.cut(d, "a.cu", "K::K").split("\n", 2)[2] == "K::K(const P* p, int n): p(p),\n    n(n) {}\n"
    assert E.cut(d, "a.cu", "K::~K").split("\n", 2)[2] == "K::~K() {}\n"


@pytest.mark.parametrize("name, text, count", [
    ("g", SRC, 0),                                     # only called, never defined
    ("f", SRC + "\nvoid f(int a) { }\n", 2),           # defined twice
    ("f", "// void f() {}\n/* void f() {} */\n", 0),   # only in comments
])
def test_refuses_missing_and_doubled_names(tmp_path, name, text, count):
    with pytest.raises(SystemExit, match=f"{name}: {count} definitions"):
        E.cut(_write(tmp_path, text), "a.cu", name)


def test_every_listed_name_is_listed_once():
    names = [n for v in E.FUNCTIONS.values() for n in v]
    assert len(names) == len(set(names)) == 26 and E.DECOMP[1] in E.FUNCTIONS[E.DECOMP[0]]
