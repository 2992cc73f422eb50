"""tests/receive_model.py against pmd.receive_batch's documented behaviour,
restated here from the oracle alone (unframe, then read_batch = inflate + UTF-8
check of text over the compressed messages, utf8_check_batch over the plain
text ones), where the two agree: no msg_max on the inflated size and
capacities that fit.  CPU only; the model is what the GPU tests of
bpmd_receive_batch compare with."""
import random

from oracle import oracle as O
from tests import frame_parse_model as FM
from tests import receive_model as M


def chain(buf, role, out_cap, inflate_cap):
    """(event, status, message) as pmd.receive_batch's docstring puts it"""
    out = bytearray(out_cap)
    s = FM.walk(buf, role, True, 0, out_cap, FM.State(), out)
    if s.event != FM.EV_MESSAGE or s.status:
        return s.event, s.status, None
    data, status = bytes(out[:s.out_len]), 0
    if s.compressed:
        status, data = O.pmd_inflate(data, cap=inflate_cap)
    if status == 0 and s.op == 1 and O.utf8_check(data) != 0:
        status = M.BAD_FRAME_PAYLOAD
    return s.event, status, data


def corpus(rng):
    texts = [b"", b"a", "grüße".encode(), "κόσμε".encode() * 40, bytes(range(32, 127)) * 30,
             b"\xc3", b"abc\x80", b"\xf4\x90\x80\x80", b"x" * 700 + b"\xe2\x82"]
    out = []
    for t in texts:
        for op in (1, 2):
            for comp in (False, True):
                for masked in (False, True):
                    payload = O.pmd_deflate(t, 6, 15, 4) if comp else t
                    fm = rng.choice([1, 7, 125, 126, 4096])
                    nf = max(1, -(-len(payload) // fm))
                    keys = [rng.getrandbits(32) for _ in range(nf)] if masked else None
                    wire = O.frame_write(payload, op, comp, keys=keys, frame_max=fm)
                    out.append((wire, FM.SERVER if masked else FM.CLIENT, t, op, comp))
    return out


def test_model_equals_the_documented_chain():
    rng = random.Random(11)
    seen = set()
    for wire, role, text, op, comp in corpus(rng):
        for cut in (0, 1):   # the whole wire, and one byte short
            buf = wire[:len(wire) - cut]
            cap = len(wire)
            want = chain(buf, role, cap, len(text) + 3)
            slot = bytearray(cap)
            e = M.receive(buf, role, True, 0, cap, len(text) + 3, FM.State(), slot)
            assert (e.stop.event, e.status) == want[:2], (text[:8], op, comp, cut)
            assert e.message == want[2]
            if cut == 0:
                assert e.stop.event == FM.EV_MESSAGE and e.message == text and e.msg_len == len(text)
                assert e.status == (M.BAD_FRAME_PAYLOAD if op == 1 and O.utf8_check(text) else 0)
                assert (e.inflated is not None) == comp
            else:
                assert (e.stop.event, e.status, e.msg_len, e.inflated) == (FM.EV_NEED_MORE, 0, 0, None)
            seen.add((e.stop.event, e.status))
    assert seen == {(FM.EV_NEED_MORE, 0), (FM.EV_MESSAGE, 0), (FM.EV_MESSAGE, M.BAD_FRAME_PAYLOAD)}


def test_model_keeps_frame_errors_and_controls():
    ping = FM.frame(b"hi", 9)
    e = M.receive(ping + FM.frame(b"x", 2), FM.CLIENT, True, 0, 8, 8, FM.State(), bytearray(8))
    assert (e.stop.event, e.status, e.msg_len, e.message, e.stop.consumed) == (FM.EV_PING, 0, 0, None, len(ping))
    e = M.receive(FM.frame(b"x", 2, rsv=2), FM.CLIENT, True, 0, 8, 8, FM.State(), bytearray(8))
    assert (e.stop.event, e.status, e.msg_len, e.message) == (FM.EV_NEED_MORE, FM.ERR["bad_reserved_bits"], 0, None)
    # zlib errors reach the status unchanged, and the message is withheld
    z = bytearray(O.pmd_deflate(b"hello hello hello hello", 6, 15, 4))
    z[0] |= 6   # block type 3
    e = M.receive(FM.frame(bytes(z), 1, rsv=4), FM.CLIENT, True, 0, 64, 64, FM.State(), bytearray(64))
    assert (e.stop.event, e.status, e.message) == (FM.EV_MESSAGE, O.pmd_inflate(bytes(z), 64)[0], None)
    assert 1 < e.status < 256
