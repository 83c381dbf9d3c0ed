"""AX.25 frames as the engine's AFSK 1200 decoder returns them (Engine.read_afsk_frames: the bytes between the flags, bit
stuffing removed, the frame check sequence checked and removed).  Host only: no device code, no library call.

    parse(frame) -> Frame(destination, source, path, control, pid, info)

An address field is 7 bytes: six characters shifted left by one bit, padded with spaces, and an SSID byte whose bits 1 ... 4 are
the SSID, whose bit 7 is the command / has-been-repeated bit and whose bit 0 ends the address list.  Callsigns are returned as
"CALL" or "CALL-SSID"; a repeater of the path that has repeated the frame carries a trailing "*".
"""
from collections import namedtuple

Frame = namedtuple("Frame", "destination source path control pid info")

MAX_REPEATERS = 8


def _address(field, repeater):
    if len(field) != 7:
        raise ValueError("AX.25: an address field of %d bytes" % len(field))
    if any(b & 1 for b in field[:6]):
        raise ValueError("AX.25: the address list ends inside a callsign")
    call = "".join(chr(b >> 1) for b in field[:6]).rstrip(" ")
    if not call or " " in call or not all(c.isdigit() or "A" <= c <= "Z" for c in call):
        raise ValueError("AX.25: %r is no callsign" % call)
    ssid = (field[6] >> 1) & 15
    text = call if ssid == 0 else "%s-%d" % (call, ssid)
    return text + ("*" if repeater and field[6] & 0x80 else ""), bool(field[6] & 1)


def parse(frame):
    """destination, source, path (a tuple of repeaters), control, pid (None unless the frame is an I or UI frame) and info of an
    AX.25 frame without its flags and FCS; ValueError on a malformed address field"""
    frame = bytes(frame)
    if len(frame) < 15:
        raise ValueError("AX.25: %d bytes hold no two addresses and a control field" % len(frame))
    destination, last = _address(frame[0:7], False)
    if last:
        raise ValueError("AX.25: the address list ends behind the destination")
    source, last = _address(frame[7:14], False)
    at, path = 14, []
    while not last:
        if len(path) == MAX_REPEATERS:
            raise ValueError("AX.25: more than %d repeaters" % MAX_REPEATERS)
        if len(frame) < at + 7 + 1:
            raise ValueError("AX.25: the address list does not end")
        hop, last = _address(frame[at:at + 7], True)
        path.append(hop)
        at += 7
    control = frame[at]
    at += 1
    pid = None
    if control & 1 == 0 or control & 0xEF == 0x03:          # I frames and UI frames carry a protocol identifier
        if len(frame) < at + 1:
            raise ValueError("AX.25: no PID behind the control field")
        pid = frame[at]
        at += 1
    return Frame(destination, source, tuple(path), control, pid, frame[at:])
