"""Test helper: the prototypes of include/sosvo.h as text -- the C types and parameter names of every entry point."""
import re

from vo_single_camera_sos_amd import _lib

_PROTOTYPES = {}


def _c_type(text):
    return " ".join(text.replace("*", " * ").split())


def prototypes():
    """{entry: (return type, [(C type, parameter name), ...])} for every function the header declares."""
    if not _PROTOTYPES:
        text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
        for m in re.finditer(r"([\w \*]+?)\b(sosvo_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
            params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
            names = [re.search(r"(\w+)\s*$", p).group(1) for p in params]
            _PROTOTYPES[m.group(2)] = (_c_type(m.group(1)), [(_c_type(p[:p.rindex(n)]), n) for p, n in zip(params, names)])
    return _PROTOTYPES


def parameter_names(entry, with_ctx=False):
    """The parameter names of a prototype of include/sosvo.h, without the context (with_ctx: every name, for the entry
    points that take no context first)."""
    names = [n for _, n in prototypes()[entry][1]]
    assert len(names) == len(_lib.SIGNATURES[entry][1])
    if with_ctx:
        return names
    assert names[0] == "ctx"
    return names[1:]
