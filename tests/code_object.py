"""The device code of a built shared library, read without a GPU: the clang offload bundles inside the file and the AMDGPU
metadata notes of their code objects.  ``library_kernels`` is the one reader of the tests and the tools."""
import os
import struct

import msgpack

from golden_util import ROOT

LIB_DIR = os.path.join(ROOT, "pytorch-yolov3_amd", "lib")
LIB = os.path.join(LIB_DIR, "libyolov3_hip.so")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(data):
    """(target triple, ELF bytes) of every device entry of every offload bundle in the file."""
    pos = 0
    while True:
        i = data.find(MAGIC, pos)
        if i < 0:
            return
        nent = struct.unpack_from("<Q", data, i + 24)[0]
        off = i + 32
        for _ in range(nent):
            o, sz, tl = struct.unpack_from("<QQQ", data, off)
            triple = data[off + 24:off + 24 + tl].decode()
            off += 24 + tl
            if sz and not triple.startswith("host"):
                yield triple, data[i + o:i + o + sz]
        pos = i + 24


def _kernels(elf):
    """amdhsa.kernels entries of one code object (NT_AMDGPU_METADATA note, msgpack)."""
    shoff = struct.unpack_from("<Q", elf, 0x28)[0]
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    for k in range(shnum):
        sh = elf[shoff + k * shentsize:shoff + (k + 1) * shentsize]
        if struct.unpack_from("<I", sh, 4)[0] != 7:          # SHT_NOTE
            continue
        so, ss = struct.unpack_from("<QQ", sh, 0x18)
        p = so
        while p < so + ss:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, p)
            d0 = p + 12 + ((namesz + 3) & ~3)
            if ntype == 32 and elf[p + 12:p + 12 + namesz].startswith(b"AMDGPU"):
                md = msgpack.unpackb(elf[d0:d0 + descsz], raw=False, strict_map_key=False)
                for kern in md.get("amdhsa.kernels", []):
                    yield kern
            p = d0 + ((descsz + 3) & ~3)


def library_path(name_or_path):
    """a file name of pytorch-yolov3_amd/lib, or a path as it is"""
    return name_or_path if os.path.dirname(name_or_path) else os.path.join(LIB_DIR, name_or_path)


def library_kernels(name_or_path="libyolov3_hip.so"):
    """the amdhsa.kernels metadata entries of every code object of a built library: there is device code, all of it for gfx950
    (one target, no multi-arch fallbacks)"""
    path = library_path(name_or_path)
    assert os.path.exists(path), "%s is not built (python -c 'import __graft_entry__ as g; g.build()')" % os.path.basename(path)
    with open(path, "rb") as f:
        objs = list(_code_objects(f.read()))
    assert objs, "no device code in %s" % os.path.basename(path)
    assert all("gfx950" in triple for triple, _ in objs), [t for t, _ in objs]
    return [k for _, elf in objs for k in _kernels(elf)]
