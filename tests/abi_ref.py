"""include/bmc_hip.h by two routes that do not pass through csrc/abi.hip: the header's own text (regular expressions) and a C
program compiled by the host C compiler.  The C-ABI tests compare the library's bmc_abi() table, and everything bmc_hip/lib.py
builds from it, with these."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
TEXT = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "bmc_hip.h")).read(), flags=re.S)      # the header without its comments


def struct_names():
    """The typedef'd structs, in the header's order."""
    return re.findall(r"^\}\s*(bmc_[a-z0-9_]+_t)\s*;", TEXT, re.M)


def constant_names():
    """Every #define BMC_* with a value (the include guard has none)."""
    return re.findall(r"^#define[ \t]+(BMC_[A-Z0-9_]+)[ \t]+\S", TEXT, re.M)


def classify(decl):
    """One parameter (or a return type) as the header writes it -> 'p' (any pointer), 'i8', 'u4', 'i4', 'f4', 'f8', or the
    name of a struct passed by value."""
    if "*" in decl or re.search(r"\bbmc_stream_t\b", decl):
        return "p"
    by_value = re.search(r"\b(bmc_[a-z0-9_]+_t)\b", decl)
    if by_value:
        return by_value.group(1)
    for words, kind in (("long long", "i8"), ("unsigned", "u4"), ("int", "i4"), ("float", "f4"), ("double", "f8")):
        if re.search(r"\b%s\b" % words, decl):
            return kind
    raise ValueError("unclassified declaration %r" % decl)


def functions():
    """{name: [class of the return type, class of each parameter, ...]} cut out of the header's declarations."""
    out = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?[a-z][a-z ]*\*?)\s*\b(bmc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", TEXT, re.M):
        params = [p.strip() for p in params.split(",")]
        out[name] = [classify(ret)] + ([] if params == ["void"] else [classify(p) for p in params])
    return out


@functools.lru_cache(maxsize=None)
def compiled(fields):
    """fields: ((struct, (field, ...)), ...) -> ({struct: (sizeof, {field: (offsetof, sizeof)})}, {constant: value}) as a C
    program compiled here with the host C compiler prints them; the constants are constant_names()."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    body = []
    for struct, names in fields:
        body.append('printf("S %s %%zu\\n", sizeof(%s));' % (struct, struct))
        body += ['printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (struct, f, struct, f, struct, f)
                 for f in names]
    body += ['printf("C %s %%.17g\\n", (double)(%s));' % (c, c) for c in constant_names()]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "bmc_hip.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(body)
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run([cc, "-I" + INCLUDE, c, "-o", exe], check=True)
        lines = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    structs, constants = {}, {}
    for kind, *rec in (line.split() for line in lines):
        if kind == "S":
            structs[rec[0]] = (int(rec[1]), {})
        elif kind == "F":
            structs[rec[0]][1][rec[1]] = (int(rec[2]), int(rec[3]))
        else:
            constants[rec[0]] = float(rec[1])
    return structs, constants


def compiled_header():
    """compiled() for the header's structs (struct_names()) with the fields the library's table names for them: a field the
    header does not have, or a struct the table lacks, fails here."""
    from bmc_hip import lib
    return compiled(tuple((s, tuple(lib.STRUCTS[s].fields)) for s in struct_names()))
