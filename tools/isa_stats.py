"""Static instruction mix of one kernel's tick loop: `python3 tools/isa_stats.py <object file> <kernel name fragment (a regex)>`.
Code object, disassembly and the kernel's record come from the build checks' reader (uav_ac/_buildcheck.py)."""
import re, collections, sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uav-autonomous-control_amd"))
from uav_ac import _buildcheck
obj=sys.argv[1]; frag=sys.argv[2]
name,ins=next((n,i) for n,i in _buildcheck._disassemble_cfg(obj).items() if n.startswith('_Z') and re.search(frag,n))
rec=next(k for k in _buildcheck.read_object(obj)["kernels"] if k.name==name)
ops=[x.split()[0] for x in ins]; addr={x.addr:i for i,x in enumerate(ins)}
br=[(i,addr[x.target],op) for i,(x,op) in enumerate(zip(ins,ops)) if (op.startswith('s_cbranch') or op=='s_branch') and x.target in addr]
bars=[i for i,op in enumerate(ops) if op=='s_barrier']
loops=[(i-t,t,i) for i,t,op in br if t<=i and (not bars or any(t<=b<=i for b in bars))]
big=[l for l in loops if l[0]>=400]; _,lo,hi=min(big) if big else max(loops)      # the tick loop: the smallest loop around a barrier that is long enough to be it (the persistent-tile loop around it is larger)
fwd=[(t-i,i,t) for i,t,op in br if lo<=i<t<=hi and op=='s_cbranch_execz']
_,olo,ohi=max(fwd)
c=collections.Counter(ops[i] for i in range(lo,hi+1) if not (olo<i<ohi))
print(name[:70])
print(' loop', hi-lo+1, 'outer', ohi-olo, 'inner', sum(c.values()), '| inner: s_mov', c['s_mov_b32'], 'lane ops', sum(v for k,v in c.items() if 'lane' in k), 'valu', sum(v for k,v in c.items() if k.startswith('v_')), 'branches', sum(v for k,v in c.items() if 'branch' in k),
      '| scalar loads', sum(v for k,v in c.items() if k.startswith('s_load')), 'waits', c['s_waitcnt'])
print(' regs:', [f"{'.'+f+':':<16} {getattr(rec,f)}" for f in ('private_segment_fixed_size','sgpr_count','sgpr_spill_count','vgpr_count','vgpr_spill_count')])
