"""ABI agreement (CPU): include/lanemap_hip.h and the ctypes table lanemapping_amd/_lib.py::SIGNATURES describe the same functions.  The
C++ sources include the header (csrc/common.h), so the compiler holds every definition to its prototype; nothing compiles the Python
table, so this test reads both: every declaration is bound and every binding declared, with the same number of parameters, each of the
same kind - int, long, unsigned, float, double or pointer - and a return value of the same kind (void and pointer included).  The
layouts of the ctypes Structures are not compared here."""
import ctypes as C
import os
import re

import pytest

from lanemapping_amd._lib import SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCALARS = {'int': 'int', 'long': 'long', 'unsigned': 'unsigned', 'unsigned int': 'unsigned', 'float': 'float', 'double': 'double', 'void': 'void'}
_CTYPES = {C.c_int: 'int', C.c_long: 'long', C.c_uint: 'unsigned', C.c_float: 'float', C.c_double: 'double', None: 'void',
           C.c_void_p: 'pointer', C.c_char_p: 'pointer'}


def c_kind(decl, named):
    """The kind of a C parameter (`named`: its last word is the parameter's name) or return type."""
    if '*' in decl or '[' in decl:
        return 'pointer'
    words = [w for w in decl.split() if w != 'const']
    if named and len(words) > 1:
        words = words[:-1]
    return _SCALARS.get(' '.join(words), f'?{decl!r}')


def ctypes_kind(t):
    if t in _CTYPES:
        return _CTYPES[t]
    return 'pointer' if isinstance(t, type) and issubclass(t, C._Pointer) else f'?{t!r}'


def declarations(text):
    """name -> (kind of the return value, [kind of each parameter]) for every function prototype of a C header."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^\s*#[^\n]*', ' ', text, flags=re.M)
    text = re.sub(r'\bextern\s*"C"\s*\{', ' ', text)
    text = re.sub(r'\b(?:typedef\s+struct|enum)\s*\w*\s*\{[^{}]*\}\s*\w*\s*;', ' ', text)
    out = {}
    for stmt in text.split(';'):
        stmt = ' '.join(stmt.split()).lstrip('} ')
        if not stmt:
            continue
        m = re.fullmatch(r'(.+?)\b(\w+)\s*\((.*)\)', stmt)
        assert m, f'not a function prototype: {stmt[:80]!r}'
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, f'{name} is declared twice'
        params = [] if params in ('', 'void') else [p.strip() for p in params.split(',')]
        out[name] = (c_kind(ret, False), [c_kind(p, True) for p in params])
    return out


def test_the_parser_reads_prototypes():
    d = declarations('''/* a comment with int f(void); in it */
        #ifndef X
        extern "C" {
        enum { A = 0, B = 1 };
        typedef struct { int a; float b[2]; } S;
        int f(void);
        const char* g(void* stream, const float* const* x, long n, unsigned k /* why */, double d, float e,
                      const S* s, int last);
        void h(void* p);   // trailing
        }
        #endif''')
    assert d == {'f': ('int', []), 'g': ('pointer', ['pointer', 'pointer', 'long', 'unsigned', 'double', 'float', 'pointer', 'int']),
                 'h': ('void', ['pointer'])}
    assert ctypes_kind(C.POINTER(C.c_double)) == 'pointer' and ctypes_kind(C.c_long) == 'long' and ctypes_kind(None) == 'void'
    assert c_kind('unsigned short v', True).startswith('?') and ctypes_kind(C.c_short).startswith('?')     # unknown kinds never compare equal silently
    with pytest.raises(AssertionError, match='not a function prototype'):
        declarations('int x = 3;')


def test_header_and_ctypes_table_agree():
    declared = declarations(open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read())
    assert len(declared) >= 119, f'{len(declared)} prototypes read from include/lanemap_hip.h: the parser lost some'
    assert set(declared) == set(SIGNATURES), (f'declared but not bound: {sorted(set(declared) - set(SIGNATURES))}; '
                                              f'bound but not declared: {sorted(set(SIGNATURES) - set(declared))}')
    bad = []
    for name, (ret, params) in sorted(declared.items()):
        res, args = SIGNATURES[name]
        bound = (ctypes_kind(res), [ctypes_kind(a) for a in args])
        unknown = [k for k in [ret, bound[0]] + params + bound[1] if k.startswith('?')]
        if unknown:
            bad.append(f'{name}: a type of no known kind: {unknown}')
        elif len(params) != len(bound[1]):
            bad.append(f'{name}: {len(params)} parameters declared, {len(bound[1])} bound')
        elif (ret, params) != bound:
            diff = [f'#{i} {a} / {b}' for i, (a, b) in enumerate(zip(params, bound[1])) if a != b]
            bad.append(f'{name}: header / binding: returns {ret} / {bound[0]}; parameters {diff}')
    assert not bad, '\n'.join(bad)
