"""include/nbasr.h as the tests read it (a helper like beam_timesteps_model.py; no tests here): the entry points it declares, and the ctypes
type the binding must give each parameter."""
import ctypes
import functools
import pathlib
import re

from nb_asr_amd import hip

HEADER = pathlib.Path(__file__).resolve().parent.parent / 'include' / 'nbasr.h'
SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong, 'size_t': ctypes.c_size_t,
           'const char*': ctypes.c_char_p}
# the two out-parameters the host itself writes are typed pointers; every other pointer is a device address and travels as c_void_p
HOST_OUT = {('nbasr_pad_amounts', 'int* left'): ctypes.POINTER(ctypes.c_int), ('nbasr_pad_amounts', 'int* right'): ctypes.POINTER(ctypes.c_int),
            ('nbasr_stream_create', 'nbasr_stream_t* stream'): ctypes.POINTER(ctypes.c_void_p)}


@functools.lru_cache(maxsize=None)
def declarations():
    """{entry point: (return type, [parameter as declared: 'type name', ...])}, comments and macros stripped."""
    code = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    code = re.sub(r'//[^\n]*|^[ \t]*#define[^\n]*', '', code, flags=re.M)
    found = {}
    for ret, name, params in re.findall(r'([\w \t]*\w[ \t\*]+)(nbasr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', code):
        params = [' '.join(p.split()) for p in params.split(',')]
        found[name] = (' '.join(ret.split()), [] if params in ([''], ['void']) else params)
    return found


def parameter_ctype(name, param):
    """The ctypes type that the binding must give one declared parameter of ``name``."""
    if (name, param) in HOST_OUT:
        return HOST_OUT[name, param]
    if param.startswith('const nbasr_deferred_ln*'):
        return ctypes.POINTER(hip.DeferredLN)
    return ctypes.c_void_p if '*' in param or param.startswith('nbasr_stream_t ') else SCALARS[param.rsplit(' ', 1)[0]]
