"""What the compiler says about include/ctd_hip.h: one gcc program for the `sizeof` of the given structs, the `offsetof`
of the given fields and the values of the given integer constants.  The layout tests compare the `_lib` mirrors and the
numpy dtypes derived from them against it."""
import os
import subprocess
import tempfile

from conftest import ROOT


def compiled_flat(structs, consts=()):
    """structs: {C type name: field names}; consts: names of integer constants.  The numbers the program prints, in order:
    per struct its `sizeof`, then the `offsetof` of every field given; then the constants."""
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "ctd_hip.h"\nint main(void){\n'
    for s, fs in structs.items():
        prog += f'printf("%zu ", sizeof({s}));\n' + "".join(f'printf("%zu ", offsetof({s}, {f}));\n' for f in fs)
    prog += "".join(f'printf("%lld ", (long long)({c}));\n' for c in consts) + "return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        with open(c, "w") as f:
            f.write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        return [int(v) for v in subprocess.check_output([exe]).split()]


def compiled(structs, consts=()):
    """`compiled_flat` by name: (sizes, offsets, values) with sizes[name] = sizeof, offsets[name] = [offsetof of every field
    given, in order], values = the constants, in order."""
    vals = compiled_flat(structs, consts)
    sizes, offsets, k = {}, {}, 0
    for s, fs in structs.items():
        sizes[s], offsets[s] = vals[k], vals[k + 1:k + 1 + len(fs)]
        k += 1 + len(fs)
    return sizes, offsets, vals[k:]
