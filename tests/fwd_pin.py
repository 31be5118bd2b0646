"""The forwarding scenarios pinned to mOS itself, shared by test_fwd_oracle.py
and golden/make_golden_fwd.py.

oracle/_ref/mos_app in "pp" mode is mOS's own ProcessPacket with everything it
sends dumped to tx.pcap (tests/test_mos_consumer.py; only the conf differs):
one monitor, forward = 1, a frozen clock.  mOS reads the kernel's route / ARP
tables only for dpdk* devices (config.c:647-772), so with `lo` the tables are
exactly the conf's.  Only one netdev can be pinned this way: every route leads
to `lo`, whose haddr is all zero.
"""
import os

import numpy as np

import fwd_oracle as F
import mosrx
import oracle_py as O
import pktlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "oracle", "_ref", "mos_app_emul")   # "pp" mode never touches the GPU stand-in
LO_ADDR = "127.0.0.1"
NOT_LOCAL = "172.16.0.1"   # the conversation traces' ICMP goes here, not to lo: mOS answers nothing itself

# /8, /16, /24, /32, a prefix-1 entry (an exact address: it ends the walk and beats the /16
# before it) and a /0 that never wins (the walk starts from prefix 0); 172.16/12 and the
# rest resolve nowhere: NO_ARP
ARP = [("10.0.0.0/8", "02:00:00:00:00:01"), ("192.168.0.0/16", "02:00:00:00:00:02"),
       ("192.168.2.27/1", "02:00:00:00:00:05"), ("192.168.1.0/24", "02:00:00:00:00:03"),
       ("192.168.9.9/32", "02:00:00:00:00:04"), ("0.0.0.0/0", "02:00:00:00:00:06")]
ROUTES = [("10.0.0.0/8", 0), ("192.168.0.0/16", 0), ("192.168.9.9/32", 0), ("0.0.0.0/0", 0)]
NETDEVS = ["00:00:00:00:00:00"]   # lo

CONF = """mos {{
	forward = 1
	netdev {{
		lo 0x0001
	}}
	mos_log = {log}/
	arp_table {{
{arp}
	}}
	route_table {{
{routes}
	}}
{nicfwd}	max_concurrency = 20000
	tcp_tw_interval = 0
	tcp_timeout = -1
}}
"""

SCENARIOS = {          # name -> (frames, nic_forward_table)
    "conv_walk": ("conv", False),
    "edge_walk": ("edge", False),
    "conv_nicfwd": ("conv", True),
}


def tables(nicfwd: bool):
    return mosrx.fwd_tables(routes=ROUTES, arp=ARP, netdevs=NETDEVS, nic_fwd={0: 0} if nicfwd else None)


def scenario_frames(kind: str):
    if kind == "conv":
        return pktlib.conversation_frames(48, seed=11, local_ip=NOT_LOCAL)
    from test_mos_consumer import fixture_frames
    return fixture_frames("edge")


def restated(frames, nicfwd: bool):
    """(buf, off, len, records, plan, tx list) of the restatement for a frame list."""
    buf, off, ln = pktlib.pack_frames(frames)
    rec = O.classify(buf, off, ln, O.params(num_msp=1, num_esp=0, forward=1, local=(LO_ADDR,)))
    t = tables(nicfwd)
    pl = F.plan(buf, off, ln, rec["reason"], t, 0, forward=1, num_msp=1, listener=False)
    n = len(off)
    cap = int(ln.astype(np.int64).sum()) + 32 * n + 16
    tx, toff, tlen, tnif, tsrc, cnt = F.build(buf, off, pl, t, cap, np.zeros(cap, np.uint8), np.zeros(n, np.uint32),
                                              np.zeros(n, np.uint16), np.zeros(n, np.int8), np.zeros(n, np.uint32))
    assert cnt[1] == 0
    return buf, off, ln, rec, pl, F.tx_list(tx, toff, tlen, int(cnt[0]))


def run_mos(tmp, name, frames, nicfwd: bool):
    """The frames mOS itself sent for the scenario (tx.pcap of a "pp" run)."""
    import subprocess
    from test_mos_consumer import pcap_frames
    d, log = tmp / f"{name}_out", tmp / f"{name}_log"
    d.mkdir()
    log.mkdir()
    conf = tmp / f"{name}.conf"
    conf.write_text(CONF.format(log=log, arp="\n".join(f"\t\t{a} {m}" for a, m in ARP),
                                routes="\n".join(f"\t\t{a} lo" for a, _ in ROUTES),
                                nicfwd="\tnic_forward_table {\n\t\tlo lo\n\t}\n" if nicfwd else ""))
    trace = tmp / f"{name}.mrxt"
    buf, off, ln = pktlib.pack_frames(frames)
    pktlib.write_ref_trace(str(trace), buf, off, ln, forward=1)
    env = dict(os.environ, MOSAPP_FROZEN_CLOCK="1")
    r = subprocess.run([APP, "pp", str(conf), str(trace), str(d)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    return pcap_frames(d / "tx.pcap")
