"""POCSAG as the engine's pager decoder reads it (include/rdsp.h "POCSAG pager decoder"; Engine.read_pocsag_messages), and as a
transmitter builds it.  Host only: no device code, no library call.

    codeword(data21), address_word(address, function), message_word(data20), SYNC, IDLE
    numeric_words(text), alpha_words(text) -> 20-bit message words;  numeric(words), alpha(words) -> text
    batches(messages) -> 32-bit words, a sync word in front of every 16;  bits(words, preamble) -> the bits, MSB first
    transmit(bits, baud, ...) -> the discriminator's output at 44 100 Hz for those bits
    from_slot(slot) -> Message, a ring slot's 84 words read

A codeword is 32 bits, MSB first on the air: bit 31 tells a message word (1) from an address word (0), 20 more data bits, ten
bits of BCH(31,21) (generator x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1) and an even parity bit.  An address word carries the
address's upper 18 bits and two function bits; the address's lower three bits are the frame, the pair of codewords 2 f and
2 f + 1 of a batch of 16, in which the address word is sent.  A message runs on from there through the codewords behind it,
across batches, up to the next address or idle word.
"""
from collections import namedtuple

import numpy as np

SYNC, IDLE, POLY = 0x7CD215D8, 0x7A89C197, 0x769
BATCH = 16
NUMERIC = "0123456789*U -)("
FLAG_CUT, FLAG_TRUNCATED, FLAG_UNCORRECTABLE = 1, 2, 4

Message = namedtuple("Message", "address function t_blocks words errors flags polarity corrected uncorrectable")


def syndrome(word):
    """the remainder of bits 31 ... 1 by the generator"""
    r = (word & 0xFFFFFFFF) >> 1
    for i in range(30, 9, -1):
        if r >> i & 1:
            r ^= POLY << (i - 10)
    return r & 0x3FF


def codeword(data21):
    d = (data21 & 0x1FFFFF) << 11
    w = d | syndrome(d) << 1
    return w | (bin(w).count("1") & 1)


def address_word(address, function=0):
    """the address word of a 21-bit address (its frame is address & 7) and a function 0 ... 3"""
    if not 0 <= address < 1 << 21 or not 0 <= function < 4:
        raise ValueError("POCSAG: address %r, function %r" % (address, function))
    return codeword((address >> 3) << 2 | function)


def message_word(data20):
    return codeword(1 << 20 | (data20 & 0xFFFFF))


def _pack(stream):
    """a list of bits, first on the air first -> 20-bit words, the last one padded with zeros"""
    stream = list(stream)
    stream += [0] * (-len(stream) % 20)
    return [int("".join(map(str, stream[k:k + 20])), 2) for k in range(0, len(stream), 20)]


def numeric_words(text):
    """4-bit BCD, least significant bit first, five characters a word, the last word padded with spaces"""
    text = text + " " * (-len(text) % 5)
    return _pack(NUMERIC.index(c) >> k & 1 for c in text for k in range(4))


def alpha_words(text):
    """7-bit characters, least significant bit first, packed without regard to the words; the last word padded with zeros"""
    data = text.encode("ascii")
    return _pack(b >> k & 1 for b in data for k in range(7))


def _unpack(words):
    return [w >> (19 - k) & 1 for w in words for k in range(20)]


def numeric(words):
    """the text of a numeric message's 20-bit words (trailing spaces are padding and stay)"""
    s = _unpack(words)
    return "".join(NUMERIC[sum(s[k + j] << j for j in range(4))] for k in range(0, len(s), 4))


def alpha(words):
    """the text of an alphanumeric message's 20-bit words, the NULs behind it left out"""
    s = _unpack(words)
    chars = [sum(s[k + j] << j for j in range(7)) for k in range(0, len(s) - 6, 7)]
    return "".join(chr(c) for c in chars).rstrip("\x00")


def batches(messages):
    """messages: (address, function, 20-bit words) each -> the transmission's 32-bit words, SYNC in front of every 16 codewords:
    every address word in its frame, idle words in every codeword not used, the last batch filled"""
    out = []

    def put(w):
        if len(out) % (BATCH + 1) == 0:
            out.append(SYNC)
        out.append(w)

    def slot():
        return (len(out) - 1) % (BATCH + 1) if len(out) % (BATCH + 1) else 0

    for address, function, words in messages:
        while slot() != 2 * (address & 7):
            put(IDLE)
        put(address_word(address, function))
        for w in words:
            put(message_word(w))
    put(IDLE)                                                                        # an idle word ends the last message
    while len(out) % (BATCH + 1):
        out.append(IDLE)
    return out


def bits(words, preamble=576):
    """a preamble of alternating bits that begins with a one, then the words, most significant bit first"""
    return [1 - k % 2 for k in range(preamble)] + [w >> (31 - k) & 1 for w in words for k in range(32)]


def transmit(stream, baud, amp=0.6, ppm=0.0, lead=0, total=None, invert=False, dc=0.0):
    """the "demod" tap of a receiver on the channel, float64 at 44 100 Hz: `lead` samples of the idle carrier (dc), then every
    bit for 44100 / (baud (1 + ppm 1e-6)) samples as -amp (a one: the lower frequency) or +amp, around dc; invert swaps the two;
    padded with the idle carrier or cut to `total` samples"""
    per = 44100.0 / (baud * (1.0 + ppm * 1e-6))
    stream = np.asarray(list(stream), np.int64)
    n = int(np.ceil(len(stream) * per))
    which = np.minimum((np.arange(n) / per).astype(np.int64), len(stream) - 1)
    x = np.where(stream[which] == 1, -amp, amp) * (-1.0 if invert else 1.0)
    out = np.full(lead + n if total is None else total, float(dc))
    k = max(0, min(n, len(out) - lead))
    out[lead:lead + k] += x[:k]
    return out


def from_slot(slot):
    """a ring slot's 84 words -> Message: words the 20 data bits of each codeword, errors the bits corrected in each (None for an
    uncorrectable one, whose data bits are as received)"""
    slot = [int(v) & 0xFFFFFFFF for v in slot]
    n, flags, pol = slot[0] & 0xFF, slot[0] >> 8 & 0xFF, slot[0] >> 16 & 1
    body = slot[4:4 + n]
    return Message(slot[2] & 0x1FFFFF, slot[2] >> 21 & 3, slot[1], [w & 0xFFFFF for w in body], [None if w >> 31 else w >> 24 & 3 for w in body], flags, pol,
                   slot[3] & 0xFFFF, slot[3] >> 16)
