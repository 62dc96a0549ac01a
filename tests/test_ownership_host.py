"""Who may call the allocator: the four runtime calls that allocate and free device and pinned memory occur in the owner's
header (csrc/kmc_mem.hip.h) and nowhere else in the library's sources, and kmc_destroy frees nothing by hand.  What the
owner does on a GPU is tests/test_ownership_gpu.py."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "k-mer-count_amd", "csrc")
OWNER = "kmc_mem.hip.h"
TOKENS = ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(")


def _sources():
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            yield name, f.read()


def test_the_allocator_is_called_in_the_owner_header_only():
    found = {t: 0 for t in TOKENS}
    elsewhere = []
    for name, text in _sources():
        for no, line in enumerate(text.splitlines(), 1):
            for t in TOKENS:
                # (hipFree( is also the tail of no other call's name; hipHostFree( does not contain it)
                if re.search(r"(?<![A-Za-z0-9_])" + re.escape(t), line):
                    if name == OWNER:
                        found[t] += 1
                    else:
                        elsewhere.append("%s:%d: %s" % (name, no, line.strip()))
    assert not elsewhere, "allocator calls outside %s:\n%s" % (OWNER, "\n".join(elsewhere))
    assert all(n == 1 for n in found.values()), found      # one place each: mem_alloc and mem_free


def _body(text, head):
    """the brace-balanced body of the function whose definition starts with `head`"""
    at = text.index(head)
    i = text.index("{", at)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i:j + 1]
        j += 1


def test_kmc_destroy_lists_no_buffers():
    text = dict(_sources())["kmc_api.hip"]
    body = _body(text, 'extern "C" void kmc_destroy(kmc_ctx* c)')
    assert "delete c;" in body and "hipStreamSynchronize" in body
    for word in ("hipFree", "hipHostFree", "free_buf", "free_keys", "free_runs", "DevBuf*", "KeyBufs*", ".reset("):
        assert word not in body, word
    assert len(body.splitlines()) <= 10


def test_owners_cannot_be_copied_and_none_is_static():
    text = dict(_sources())[OWNER]
    assert "Mem(const Mem&) = delete;" in text and "Mem& operator=(const Mem&) = delete;" in text
    for name, src in _sources():
        for no, line in enumerate(src.splitlines(), 1):
            if re.search(r"\b(static|thread_local)\b[^;(]*\b(Dev|Pin|Mem)<|\b(static|thread_local)\b[^;(]*\b(DevBuf|KeyBufs|Table|Run|Pinned)\b\s+\w+\s*[;={\[]", line):
                raise AssertionError("%s:%d: an owner with static storage: %s" % (name, no, line.strip()))


def test_debug_mem_is_exported_beside_the_abi(kmc):
    assert "kmc_debug_mem" not in kmc.ABI_SYMBOLS
    with open(os.path.join(ROOT, "include", "kmc.h")) as f:
        assert "kmc_debug_mem" not in f.read()
    # (the counters are the process's own; no ctx has been opened by the library in a process without a GPU, and every
    # ctx another test of this process opened is closed or still counted -- the call itself needs no device)
    m = kmc.debug_mem()
    assert len(m) == 5 and all(isinstance(v, int) and v >= 0 for v in m) and m[4] == 0
