"""Hand-traced known answers of the client side (KAT_CLIENT), worked from the Go text of
genericsmr.(*Replica).clientListener (genericsmr.go:448-490) and the Unmarshals it calls: each
case gives the connections' bytes as hex, their groups, and what the reference frames from them:
per connection (proposals [(CommandId, Op, K, V, Timestamp)], dropped frames, consumed bytes,
stop reason, stop code), then prop_off and send_off for n_groups.

Reading a frame by hand: the code byte, then little-endian fields. PROPOSE (0): CommandId 4, Op 1,
K 8, V 8, Timestamp 8 = 30 bytes with the code. READ (2): CommandId 4, Key 8 = 13. PROPOSE_AND_READ
(4): CommandId 4, Command 17, Key 8 = 30. Any other code: the switch falls through, 1 byte."""
END, PARTIAL = 0, 1
I64_MIN = -(1 << 63)

_Z30 = "00" * 30
_P1 = "00" "07000000" "01" "0a00000000000000" "1400000000000000" "e803000000000000"  # id 7 PUT 10 20 ts 1000
_P2 = "00" "08000000" "02" "0b00000000000000" "0000000000000000" "e903000000000000"  # id 8 GET 11 0 ts 1001
_R = "02" "09000000" "0c00000000000000"                                               # READ id 9 key 12
_PAR = "04" "0a000000" "01" "0d00000000000000" "0e00000000000000" "0f00000000000000"  # P&R id 10
_UNKNOWN = "".join("%02x" % c for c in range(256) if c not in (0, 2, 4))

KAT_CLIENT = [
    dict(name="extremes",
         # CommandId ff ff ff ff = -1; Op 01; K 00..00 80 = INT64_MIN; V ff x8 = -1;
         # Timestamp 01 00 .. 00 80 = INT64_MIN + 1 (top bit set)
         conns=["00" "ffffffff" "01" "0000000000000080" "ffffffffffffffff" "0100000000000080"],
         groups=[0], n_groups=1,
         want=[([(-1, 1, I64_MIN, -1, I64_MIN + 1)], 0, 30, END, -1)],
         prop_off=[0, 1], send_off=[0, 1]),
    dict(name="all_zero_payloads",
         # 60 zero bytes: byte 0 is PROPOSE, its 29 payload bytes are zero; byte 30 the same
         conns=[_Z30 + _Z30], groups=[0], n_groups=1,
         want=[([(0, 0, 0, 0, 0), (0, 0, 0, 0, 0)], 0, 60, END, -1)],
         prop_off=[0, 2], send_off=[0, 1]),
    dict(name="payload_of_2_and_4",
         # a Propose whose payload bytes are the codes READ and PROPOSE_AND_READ, then a Read whose
         # payload bytes are 4: nothing inside a payload is read as a code
         conns=["00" "02040204" "02" "0402040204020402" "0202020202020202" "0404040404040404"
                "02" "04040404" "0404040404040404"],
         groups=[0], n_groups=1,
         want=[([(0x04020402, 2, 0x0204020402040204, 0x0202020202020202, 0x0404040404040404)],
                1, 43, END, -1)],
         prop_off=[0, 1], send_off=[0, 1]),
    dict(name="every_unknown_code",
         # 1, 3, 5..255: 253 one-byte frames
         conns=[_UNKNOWN], groups=[0], n_groups=1,
         want=[([], 253, 253, END, -1)], prop_off=[0, 0], send_off=[0, 0]),
    dict(name="read_and_par_between_proposes",
         conns=[_P1 + _R + _PAR + _P2], groups=[0], n_groups=1,
         want=[([(7, 1, 10, 20, 1000), (8, 2, 11, 0, 1001)], 2, 103, END, -1)],
         prop_off=[0, 2], send_off=[0, 1]),
    dict(name="propose_one_byte_short",
         conns=[_P1[:58]], groups=[0], n_groups=1,
         want=[([], 0, 0, PARTIAL, 0)], prop_off=[0, 0], send_off=[0, 0]),
    dict(name="propose_then_short_read",
         conns=[_P1 + _R[:10]], groups=[0], n_groups=1,
         want=[([(7, 1, 10, 20, 1000)], 0, 30, PARTIAL, 2)], prop_off=[0, 1], send_off=[0, 1]),
    dict(name="unknown_then_short_par",
         conns=["07" + _PAR[:20]], groups=[0], n_groups=1,
         want=[([], 1, 1, PARTIAL, 4)], prop_off=[0, 0], send_off=[0, 0]),
    dict(name="empty_connection",
         conns=[""], groups=[0], n_groups=1,
         want=[([], 0, 0, END, -1)], prop_off=[0, 0], send_off=[0, 0]),
    dict(name="short_inside_the_command",
         # code, CommandId and 10 of the Command's 17 bytes: the reference ignores the Command's
         # error and desynchronises; the engine (and the model) keep the tail from the code byte
         conns=[_P1[:30]], groups=[0], n_groups=1,
         want=[([], 0, 0, PARTIAL, 0)], prop_off=[0, 0], send_off=[0, 0]),
    dict(name="unknown_byte_shifts_the_frames",
         conns=["07" + _P2], groups=[0], n_groups=1,
         want=[([(8, 2, 11, 0, 1001)], 1, 31, END, -1)], prop_off=[0, 1], send_off=[0, 1]),
    dict(name="groups_with_holes",
         # groups 0 and 2 of 4: group 1 and group 3 have no connection
         conns=[_P1, _P2 + _P1, "", _R[:4]], groups=[0, 2, 2, 2], n_groups=4,
         want=[([(7, 1, 10, 20, 1000)], 0, 30, END, -1),
               ([(8, 2, 11, 0, 1001), (7, 1, 10, 20, 1000)], 0, 60, END, -1),
               ([], 0, 0, END, -1),
               ([], 0, 0, PARTIAL, 2)],
         prop_off=[0, 1, 1, 3, 3], send_off=[0, 1, 1, 2, 2]),
]


def kat_bytes(case):
    return [bytes.fromhex(h) for h in case["conns"]]
