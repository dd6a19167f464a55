"""A stand-in for the ``warp`` module: the reference's Warp kernels as plain Python on the CPU.

TEST INFRASTRUCTURE ONLY (tests/golden/make_warp_golden.py, tests/test_warp_standin.py).  The
product path never imports ``oracle/``.

The reference's kernels (thesis_master/warp_implementation/*.py) use 25 names of Warp and its host
class 11 more.  ``create()`` returns a module object that offers exactly those, so that the
reference's own files import and run unchanged with it in ``sys.modules["warp"]``: the launch
order, the arguments and the resets are then the reference's, not a restatement.  It DEFINES
(DESIGN.md §4 D16):

  arithmetic  every float value is a numpy float32 scalar, so every + - * / is one IEEE float32
              operation in source order: no contraction, no double intermediate.  With numpy >= 2 a
              Python literal next to a float32 stays float32, as a literal does inside a kernel.
              ``dot`` is accumulated left to right, ``cross`` rounds both products of a component.
  small types vec2f, vec3f, mat22f hold float32 components; reading one from an array is a copy.
              ``int`` truncates toward zero, ``float`` / ``float32`` round to float32.
  launch      arguments are converted by the kernel's annotations (``float`` -> float32, ``int`` ->
              Python int); the threads run one after the other in ascending ``tid``.  ``func``
              converts the same way.
  arrays      a wrapper over numpy that checks bounds: a negative or too large index raises
              IndexError, it never wraps.  (The reference reads out of bounds outside the map; what
              the project does there is its own choice, D3, so a fixture must stay inside.)
  math        sin, cos, exp, atan, pow come from a table chosen at creation:
              "project"  oracle.dmath (the definition under which bits can be compared; CUDA's sinf
                         / expf cannot be reproduced offline).  pow is defined for the exponent 1.0
                         alone (the one the kernels use: x itself); atan is not defined (no launched
                         kernel calls it, D10) and raises.
              "libm"     float64 libm rounded once to float32.
  randn       ``randn(state)`` is ``randn_table[state]`` of a float32 table the caller supplies; every
              state asked for is appended to ``randn_states``.
  atomics     ``atomic_add`` adds in float32, ``atomic_min`` takes the smaller, both in launch order.
"""
from __future__ import annotations

import builtins
import math
import types

import numpy as np

from . import dmath

F32 = np.float32


# ============================================================== small types
class _Vec:
    """n float32 components; value semantics (every operation returns a new one)."""
    N = 0
    __array_ufunc__ = None          # numpy scalars defer to __rmul__ instead of broadcasting
    __slots__ = ("c",)

    def __init__(self, *a):
        if len(a) == 1 and not np.isscalar(a[0]):
            a = tuple(a[0].c) if isinstance(a[0], _Vec) else tuple(a[0])
        if len(a) == 0:
            a = (0.0,) * self.N
        if len(a) != self.N:
            raise TypeError(f"{type(self).__name__} takes {self.N} components, got {len(a)}")
        self.c = [F32(x) for x in a]

    def _new(self, comps):
        v = type(self).__new__(type(self))
        v.c = list(comps)
        return v

    def _same(self, o):
        if type(o) is not type(self):
            raise TypeError(f"{type(self).__name__} with {type(o).__name__}")
        return o

    def __getitem__(self, i):
        if not 0 <= i < self.N:
            raise IndexError(f"component {i} of {type(self).__name__}")
        return self.c[i]

    def __setitem__(self, i, x):
        if not 0 <= i < self.N:
            raise IndexError(f"component {i} of {type(self).__name__}")
        self.c[i] = F32(x)

    def __len__(self):
        return self.N

    def __iter__(self):
        return iter(self.c)

    def __add__(self, o):
        return self._new(a + b for a, b in zip(self.c, self._same(o).c))

    def __sub__(self, o):
        return self._new(a - b for a, b in zip(self.c, self._same(o).c))

    def __mul__(self, s):
        s = F32(s)
        return self._new(a * s for a in self.c)

    def __rmul__(self, s):
        s = F32(s)
        return self._new(s * a for a in self.c)

    def __truediv__(self, s):
        s = F32(s)
        return self._new(a / s for a in self.c)

    def __neg__(self):
        return self._new(-a for a in self.c)

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(repr(float(a)) for a in self.c)})"


class vec2f(_Vec):
    N = 2
    __slots__ = ()


class vec3f(_Vec):
    N = 3
    __slots__ = ()


class mat22f:
    """2 x 2 float32, indexed m[i, j]."""
    __array_ufunc__ = None
    __slots__ = ("m",)

    def __init__(self, *a):
        if len(a) == 1:
            a = tuple(np.asarray(a[0], F32).reshape(-1))
        if len(a) == 0:
            a = (0.0,) * 4
        if len(a) != 4:
            raise TypeError("mat22f takes 4 components")
        self.m = [F32(x) for x in a]

    @staticmethod
    def _at(ij):
        i, j = ij
        if not (0 <= i < 2 and 0 <= j < 2):
            raise IndexError(f"element {ij} of mat22f")
        return 2 * i + j

    def __getitem__(self, ij):
        return self.m[self._at(ij)]

    def __setitem__(self, ij, x):
        self.m[self._at(ij)] = F32(x)


_SHAPES = {vec2f: (2,), vec3f: (3,), mat22f: (2, 2)}


def _element(dtype):
    """The element kind of an array dtype: "f" (float32 scalar) or one of the small types."""
    if dtype in _SHAPES:
        return dtype
    if dtype is builtins.float or getattr(dtype, "_standin_scalar", None) == "f":
        return "f"
    raise TypeError(f"array dtype {dtype!r} is not offered by the stand-in")


# ============================================================== arrays
class array:
    """``array(data, dtype=...)``: a bounds-checked 1-D array.  ``array(dtype=..., ndim=...)`` without
    data is the annotation of a kernel argument."""

    def __init__(self, data=None, dtype=builtins.float, ndim=None, device=None, **_):
        self.dtype = dtype
        self.kind = _element(dtype)
        if data is None:
            self.a = None           # an annotation
            return
        tail = _SHAPES.get(self.kind, ())
        if isinstance(data, np.ndarray):
            a = np.array(data, dtype=F32)
        else:
            a = np.array([tuple(x.c) if isinstance(x, _Vec) else (x.m if isinstance(x, mat22f) else x)
                          for x in data], dtype=F32)
        self.a = np.ascontiguousarray(a.reshape((-1,) + tail))

    @property
    def shape(self):
        return (self.a.shape[0],)

    def __len__(self):
        return self.a.shape[0]

    def _index(self, i):
        if isinstance(i, (bool, np.bool_)) or not isinstance(i, (builtins.int, np.integer)):
            raise TypeError(f"array index must be an integer, got {type(i).__name__}")
        if not 0 <= i < self.a.shape[0]:
            raise IndexError(f"index {i} outside an array of {self.a.shape[0]} elements")
        return builtins.int(i)

    def __getitem__(self, i):
        i = self._index(i)
        if self.kind == "f":
            return self.a[i]
        return self.kind(self.a[i])                    # a copy

    def __setitem__(self, i, x):
        i = self._index(i)
        if self.kind == "f":
            self.a[i] = F32(x)
        elif self.kind is mat22f:
            if not isinstance(x, mat22f):
                raise TypeError("mat22f array takes mat22f")
            self.a[i] = np.array(x.m, F32).reshape(2, 2)
        else:
            if type(x) is not self.kind:
                raise TypeError(f"{self.kind.__name__} array takes {self.kind.__name__}, got {type(x).__name__}")
            self.a[i] = x.c

    def numpy(self):
        return self.a.copy()

    def zero_(self):
        self.a[...] = 0

    def assign(self, src):
        src = src.a if isinstance(src, array) else np.asarray(src, F32)
        self.a[...] = src.reshape(self.a.shape)


def zeros(shape, dtype=builtins.float, device=None, **_):
    n = builtins.int(shape[0] if isinstance(shape, (tuple, list)) else shape)
    return array(np.zeros((n,) + _SHAPES.get(_element(dtype), ()), F32), dtype=dtype)


# ============================================================== kernels
def _converter(ann):
    if ann is builtins.float or getattr(ann, "_standin_scalar", None) == "f":
        return F32
    if ann is builtins.int or getattr(ann, "_standin_scalar", None) == "i":
        def to_int(x):
            if builtins.int(x) != x:
                raise TypeError(f"int argument got {x!r}")
            return builtins.int(x)
        return to_int
    if ann in _SHAPES:
        def to_small(x, ann=ann):
            if type(x) is not ann:
                raise TypeError(f"{ann.__name__} argument got {type(x).__name__}")
            return ann(x) if ann is not mat22f else mat22f(x.m)
        return to_small
    if isinstance(ann, array):
        def to_array(x, ann=ann):
            if not isinstance(x, array) or x.a is None:
                raise TypeError(f"array argument got {type(x).__name__}")
            if x.kind != ann.kind:
                raise TypeError("array argument of another dtype")
            return x
        return to_array
    return lambda x: x


def _converters(fn):
    names = fn.__code__.co_varnames[:fn.__code__.co_argcount]
    ann = fn.__annotations__
    return [_converter(ann.get(n)) for n in names]


class Kernel:
    def __init__(self, fn):
        self.fn = fn
        self.__name__ = fn.__name__
        self.conv = _converters(fn)


def kernel(fn):
    return Kernel(fn)


def func(fn):
    conv = _converters(fn)

    def call(*args):
        if len(args) != len(conv):
            raise TypeError(f"{fn.__name__} takes {len(conv)} arguments, got {len(args)}")
        return fn(*[c(a) for c, a in zip(conv, args)])

    call.__name__ = fn.__name__
    call.__wrapped__ = fn
    return call


def _scalar(kind, f):
    f._standin_scalar = kind
    return f


TABLES = ("project", "libm")


def _math_table(name):
    if name == "project":
        def no_atan(x):
            raise NotImplementedError("the project defines no float32 atan (DESIGN.md §4 D10)")

        def pow1(x, y):
            if F32(y) != F32(1.0):
                raise NotImplementedError("the project defines pow for the exponent 1.0 alone")
            return F32(x)

        return dict(sin=lambda x: F32(dmath.dm_sincosf(F32(x))[0]), cos=lambda x: F32(dmath.dm_sincosf(F32(x))[1]),
                    exp=lambda x: F32(dmath.dm_expf(F32(x))), atan=no_atan, pow=pow1)
    if name == "libm":
        def exp(x):
            try:
                return F32(math.exp(builtins.float(x)))
            except OverflowError:
                return F32(np.inf)

        return dict(sin=lambda x: F32(math.sin(builtins.float(x))), cos=lambda x: F32(math.cos(builtins.float(x))),
                    exp=exp, atan=lambda x: F32(math.atan(builtins.float(x))),
                    pow=lambda x, y: F32(math.pow(builtins.float(F32(x)), builtins.float(F32(y)))))
    raise ValueError(f"math table {name!r}: one of {TABLES}")


def create(math_table="project", randn_table=None):
    """A fresh ``warp`` module object.  ``randn_table`` may be set later (``wp.randn_table = ...``)."""
    wp = types.ModuleType("warp")
    wp.__doc__ = "oracle.warp_standin: the reference's Warp names on the CPU, float32, in launch order"
    wp.math_table = math_table
    tab = _math_table(math_table)
    wp.randn_table = None if randn_table is None else np.asarray(randn_table, F32)
    wp.randn_states = []
    state = {"tid": None}

    # ---- declarations and host side
    wp.func, wp.kernel, wp.array, wp.zeros = func, kernel, array, zeros
    wp.vec2f, wp.vec3f, wp.mat22f = vec2f, vec3f, mat22f
    wp.init = lambda: None

    def launch(kernel=None, dim=None, inputs=(), outputs=(), device=None, **_):
        if not isinstance(kernel, Kernel):
            raise TypeError("launch needs a function declared with wp.kernel")
        args = list(inputs) + list(outputs)
        if len(args) != len(kernel.conv):
            raise TypeError(f"{kernel.__name__} takes {len(kernel.conv)} arguments, got {len(args)}")
        args = [c(a) for c, a in zip(kernel.conv, args)]
        if state["tid"] is not None:
            raise RuntimeError("launch inside a kernel")
        try:
            for t in range(builtins.int(dim)):
                state["tid"] = t
                # small-type arguments are per-thread values
                kernel.fn(*[type(a)(a) if isinstance(a, _Vec) else a for a in args])
        finally:
            state["tid"] = None

    def tid():
        if state["tid"] is None:
            raise RuntimeError("tid() outside a launch")
        return state["tid"]

    wp.launch, wp.tid = launch, tid

    # ---- scalar types
    wp.int = _scalar("i", lambda x: builtins.int(x))               # toward zero
    wp.float = _scalar("f", lambda x: F32(x))
    wp.float32 = _scalar("f", lambda x: F32(x))
    wp.uint32 = _scalar("i", lambda x: builtins.int(x) & 0xFFFFFFFF)

    # ---- arithmetic
    wp.sqrt = lambda x: F32(np.sqrt(F32(x)))
    wp.abs = lambda x: F32(np.abs(F32(x)))
    wp.trunc = lambda x: F32(np.trunc(F32(x)))

    def clamp(x, lo, hi):
        x, lo, hi = F32(x), F32(lo), F32(hi)
        return builtins.min(builtins.max(lo, x), hi)           # min(max(a, x), b)

    def dot(a, b):
        a._same(b)
        s = a.c[0] * b.c[0]
        for i in range(1, a.N):
            s = s + a.c[i] * b.c[i]
        return s

    def cross(a, b):
        if type(a) is not vec3f or type(b) is not vec3f:
            raise TypeError("cross takes two vec3f")
        a, b = a.c, b.c
        return vec3f(a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])

    wp.clamp, wp.dot, wp.cross = clamp, dot, cross
    for name in ("sin", "cos", "exp", "atan", "pow"):
        setattr(wp, name, tab[name])

    # ---- noise and atomics
    def randn(s):
        s = builtins.int(s)
        wp.randn_states.append(s)
        if wp.randn_table is None:
            raise RuntimeError("randn needs a randn_table")
        if not 0 <= s < len(wp.randn_table):
            raise IndexError(f"randn state {s} outside the table of {len(wp.randn_table)}")
        return F32(wp.randn_table[s])

    def atomic_add(arr, i, v):
        old = arr[i]
        arr[i] = old + F32(v)
        return old

    def atomic_min(arr, i, v):
        old = arr[i]
        v = F32(v)
        if v < old:
            arr[i] = v
        return old

    wp.randn, wp.atomic_add, wp.atomic_min = randn, atomic_add, atomic_min
    return wp
