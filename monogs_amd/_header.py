"""Reader of include/monogs_raster.h: the C ABI is stated once, in the header, and the ctypes binding (_lib.py) is derived from it.

Standard library and ctypes only.  The reader knows exactly the constructs the header uses -- ``typedef struct TAG { ... } NAME;``,
one anonymous ``enum { ... };``, ``#define MGS_NAME <expression>``, function declarations, the ``extern "C"`` brackets -- and fails
loudly on anything else: text it did not consume, an unknown type name or a declarator it cannot read raises `HeaderError` naming
the line; a declaration is never skipped.  Scalars map to the ctypes type of the same width (`SCALARS`).  In a struct a pointer is
``c_void_p`` and ``T name[N]`` is ``T * N``.  A parameter that points to a struct of the header is ``POINTER(that class)``, a
``const char*`` parameter or result is ``c_char_p``, every other pointer (``T**`` too) is ``c_void_p``: the header cannot tell host
from device pointers, and ``c_void_p`` takes ``byref(...)``, ctypes arrays, integers and None alike.  Classes: typedefs in CamelCase.
"""
import ctypes as C
import functools
import operator
import os
import re
import types

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monogs_raster.h")

SCALARS = {"int": C.c_int, "int16_t": C.c_int16, "uint16_t": C.c_uint16, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
           "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
           "uint8_t": C.c_uint8, "unsigned long long": C.c_ulonglong}
_DECLARATOR = re.compile(r"(const\s+)?(unsigned long long|\w+)\b((?:\*|\bconst\b|\s)*)(\w+)\s*(?:\[\s*(\d+)\s*\])?$")
_SPACE = re.compile(r"\s*")
_STRUCT = re.compile(r"typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;")
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;")
_ENUMERATOR = re.compile(r"(\w+)\s*(?:=\s*(\S.*?))?\s*", re.S)
_EXTERN_C = re.compile(r'extern\s+"C"\s*\{')
_FUNCTION = re.compile(r"([^()]*?\w)\s*\(([^()]*)\)\s*", re.S)
_DEFINE = re.compile(r"#\s*define\s+(MGS_\w+)\s+(\S.*)$")
_OTHER_DIRECTIVE = re.compile(r"#\s*(?:(?:if|ifdef|ifndef|else|endif|include)\b.*|define\s+\w+\s*)$")
_TOKEN = re.compile(r"\s*(?:(0[xX][0-9a-fA-F]+|\d+)[uUlL]*(?![\w.])|((?:\d+\.\d*|\.\d+)(?:[eE][-+]?\d+)?|\d+[eE][-+]?\d+)[fF]?(?!\w)"
                    r"|([A-Za-z_]\w*)|(<<|>>|[-+*|()]))")            # an integer, a float, a name or an operator
_BINARY = ({"|": operator.or_}, {"<<": operator.lshift, ">>": operator.rshift}, {"+": operator.add, "-": operator.sub},
           {"*": operator.mul})                                # the binary operators by C's precedence, loosest first


class HeaderError(ValueError):
    """The header holds something the reader does not know; the message names the line."""


def _evaluate(expr: str, known: dict, fail):
    """Value of a #define's or enumerator's expression: integer and float literals (u / l / f suffixes), earlier names,
    ``* + - << >> |`` and parentheses.  A small evaluator of its own: the file's text never reaches the interpreter."""
    tokens, pos = [], 0
    while expr[pos:].strip():
        m = _TOKEN.match(expr, pos) or fail(f"cannot read the expression at {expr[pos:].strip()!r}")
        integer, real, name, op = m.groups()
        tokens.append(int(integer, 0) if integer else float(real) if real else name or op)
        pos = m.end()

    def atom():
        t = tokens.pop(0) if tokens else fail("the expression ends early")
        if t == "(":
            v = binary(0)
            return v if tokens and tokens.pop(0) == ")" else fail("unbalanced parentheses")
        if isinstance(t, str):
            return known[t] if t in known else fail(f"{t!r} is not an earlier constant")
        return t

    def binary(level):
        if level == len(_BINARY):
            return atom()
        v = binary(level + 1)
        while tokens and tokens[0] in _BINARY[level]:
            v = _BINARY[level][tokens.pop(0)](v, binary(level + 1))
        return v

    try:
        value = binary(0)
    except TypeError:
        fail("an integer operator on a float")
    return fail(f"unexpected {tokens[0]!r} in the expression") if tokens else value


def parse(text: str, origin: str = "header") -> types.SimpleNamespace:
    """``structs``: Python class name -> ctypes.Structure subclass, in the header's order; ``functions``: symbol -> (restype,
    [argtypes]); ``constants``: a namespace of every #define MGS_* and every enumerator, int or float."""
    def fail_at(pos, why):
        line = text.count("\n", 0, pos) + 1
        raise HeaderError(f"{origin}:{line}: {why}: {text.splitlines()[line - 1].strip()!r}")

    blank = lambda m: re.sub(r"[^\n]+", lambda run: " " * len(run.group()), m.group())  # noqa: E731  (offsets and lines survive)
    src = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)
    structs, functions, constants, by_c_name = {}, {}, {}, {}

    def define(name, expr, value, pos):
        if name in constants:
            fail_at(pos, f"{name} is defined twice")
        constants[name] = _evaluate(expr, constants, lambda why: fail_at(pos, why)) if expr else value

    def directive(m):
        line, pos = m.group().strip(), m.end() - len(m.group().lstrip())
        d = _DEFINE.match(line)
        if d:
            define(d.group(1), d.group(2), None, pos)
        elif not _OTHER_DIRECTIVE.match(line):
            fail_at(pos, "a preprocessor line the reader does not know")
        return blank(m)
    src = re.sub(r"^[ \t]*#[^\n]*", directive, src, flags=re.M)

    def declare(piece, pos, role):
        """``T name``, ``T* name`` or (fields) ``T name[N]`` -> (name, ctypes type) by the rules of a field, parameter or result."""
        m = _DECLARATOR.match(piece.strip()) or fail_at(pos, "a declarator the reader cannot read")
        const, base, middle, name, count = m.groups()
        stars = middle.count("*")
        if base not in SCALARS and not (stars and (base in by_c_name or base in ("void", "char"))):
            fail_at(pos, f"unknown (or by-value) type {base!r}")
        if count and role != "field":
            fail_at(pos, "an array outside a struct")
        ctype = C.c_void_p if stars else SCALARS[base]
        if stars == 1 and base == "char" and const and role != "field":
            ctype = C.c_char_p
        elif stars == 1 and base in by_c_name and role == "parameter":
            ctype = C.POINTER(by_c_name[base])
        return name, ctype * int(count) if count else ctype

    def pieces(body, start, separator):
        return [(m.group(), start + m.start()) for m in re.finditer(r"[^\s%s][^%s]*" % (separator, separator), body)]

    pos, extern_c = _SPACE.match(src).end(), False
    while pos < len(src):
        m = _EXTERN_C.match(src, pos)
        if m or (extern_c and src[pos] == "}"):
            extern_c, end = bool(m), m.end() if m else pos + 1
        elif src.startswith("typedef", pos):
            m = _STRUCT.match(src, pos) or fail_at(pos, "an unterminated struct, or a typedef the reader does not know")
            fields, end = [], m.end()
            for statement, at in pieces(m.group(1), m.start(1), ";"):
                head = _DECLARATOR.match(statement.split(",")[0].strip())       # `int32_t width, height;`: the type is the first's
                prefix = f"{head.group(1) or ''}{head.group(2)} " if head else ""
                for k, (piece, p) in enumerate(pieces(statement, at, ",")):
                    fields.append(declare(prefix + piece if k else piece, p, "field"))
            c_name = m.group(2)                                                  # mgs_camera -> MgsCamera, MgsStereo stays
            py_name = c_name if c_name != c_name.lower() else "".join(part.capitalize() for part in c_name.split("_"))
            by_c_name[c_name] = structs[py_name] = type(py_name, (C.Structure,), {"_fields_": fields})
        elif src.startswith("enum", pos):
            m = _ENUM.match(src, pos) or fail_at(pos, "an enum the reader does not know")
            value, end = -1, m.end()
            for piece, p in pieces(m.group(1), m.start(1), ","):
                e = _ENUMERATOR.fullmatch(piece) or fail_at(p, "an enumerator the reader cannot read")
                define(e.group(1), e.group(2), value + 1, p)
                value = constants[e.group(1)]
        else:
            end = src.find(";", pos) + 1
            m = (_FUNCTION.fullmatch(src, pos, end - 1) if end else None) or fail_at(pos, "text that is no declaration the reader knows")
            name, restype = declare(m.group(1), pos, "result")
            params = [] if m.group(2).strip() == "void" else pieces(m.group(2), m.start(2), ",")
            functions[name] = (restype, [declare(piece, p, "parameter")[1] for piece, p in params])
        pos = _SPACE.match(src, end).end()
    return types.SimpleNamespace(structs=structs, functions=functions, constants=types.SimpleNamespace(**constants))


@functools.lru_cache(maxsize=None)
def read(path: str = HEADER_PATH) -> types.SimpleNamespace:
    """The parsed header (once per path and process)."""
    with open(path) as f:
        return parse(f.read(), os.path.basename(path))
