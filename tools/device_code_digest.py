"""Per-kernel digest of the device code of csrc/*.hip, to prove that a host-only change left every kernel as it was.

    python tools/device_code_digest.py [CSRC_DIR] > digest.txt        (then diff two digests)

Each source is compiled for the device alone with the build's own flags; for every FUNC symbol of the code object one
line "file name size sha256(bytes)" is printed, and for every kernel descriptor (*.kd) its hash with bytes 16-23 (the
entry offset, which moves with the order of emission) zeroed.  __hip_cuid_* changes with the source text and is left out.
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sincformer_metacog_speech_enhancement_amd import build as B  # noqa: E402


def symbols(elf):
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    for _, typ, _, _, off, size, link, _, _, entsize in sec:
        if typ != 2:                                        # SHT_SYMTAB
            continue
        stroff = sec[link][4]
        for o in range(off, off + size, entsize):
            name, info, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", elf, o)
            name = elf[stroff + name:elf.index(b"\0", stroff + name)].decode()
            if 0 < shndx < shnum and sec[shndx][1] != 8:    # defined, not in a NOBITS section
                start = sec[shndx][4] + value - sec[shndx][3]
                yield name, info & 15, ssize, bytearray(elf[start:start + ssize])


def digest(csrc, src):
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "dev.o")
        flags = [csrc if f == B.CSRC else f for f in B.FLAGS] + B.EXTRA.get(src, [])
        subprocess.run([B.HIPCC] + flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-w", "-c",
                                            os.path.join(csrc, src), "-o", obj], check=True)
        elf = open(obj, "rb").read()
    lines = []
    for name, typ, size, data in symbols(elf):
        if name.startswith("__hip_cuid_"):
            continue
        if name.endswith(".kd"):
            data[16:24] = bytes(8)
        elif typ != 2:                                      # STT_FUNC
            continue
        lines.append("%s %s %d %s" % (src, name, size, hashlib.sha256(data).hexdigest()))
    return sorted(lines)


if __name__ == "__main__":
    csrc = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else B.CSRC
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=6) as ex:
        for src, lines in zip(srcs, ex.map(lambda s: digest(csrc, s), srcs)):
            print("\n".join(lines) if lines else "%s (no device code)" % src)
