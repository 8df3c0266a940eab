#!/bin/bash
# usage: bash profiles/ab.sh "<variant> <variant> ..." "<env batch outputs traj [extra bench args]>" ...
# Same-box A/B of kernel library builds (neorl-industrial-gym_amd/libnig_<variant>.so, built by hand):
# box-to-box spread of the fused rollout is ~15 %, larger than most single optimisations.
# NIG_AB_ROUNDS (default 2): fresh processes per variant and configuration; the variants alternate within every round.
# Per run: rate, launch time, roofline fraction, ms_per_step, the shader clock held over the timed launches, package power,
# and shader cycles per env-step (= launch_us x MHz / steps per launch).
export NIG_NO_AUTOBUILD=1
variants=$1; shift
cfgs=("$@")
# a variant is loaded through NIG_LIB_PATH: libnig.so itself is never overwritten ("base" = the built libnig.so)
for r in $(seq 1 ${NIG_AB_ROUNDS:-2}); do for v in $variants; do
  if [ "$v" = base ]; then unset NIG_LIB_PATH; else export NIG_LIB_PATH=$PWD/neorl-industrial-gym_amd/libnig_$v.so; fi
  for cfg in "${cfgs[@]}"; do read -r e b o t extra <<< "$cfg"; echo -n "$v $cfg: "
    timeout -k 10 100 python bench.py --env $e --batch $b --outputs $o --traj $t --steps 40 --warmup 8 --settle 0.4 --no-cpu-baseline --no-step-api --no-parity --no-powergrid --no-mixed --no-robotassembly --no-brackets $extra 2>/dev/null | python -c "
import json,sys; d=json.load(sys.stdin); rt=d.get('rank_times',{}); mhz=rt.get('clock',{}).get('shader_clock_mhz'); w=rt.get('dpm',{}).get('power_w'); us=d['roofline']['launch_us']; P=d['config']['plan_steps']
print('%.3e  launch_us %.1f  frac %.3f  ms_per_step %.4f  clock_mhz %s  power_w %s  cycles_per_env_step %s' % (d['value'], us, d['roofline']['frac'], d['ms_per_step'], '%.0f' % mhz if mhz else '-', '%.0f' % w if w else '-', '%.0f' % (us * mhz / P) if mhz else '-'))" || exit 1
  done
done; done
unset NIG_LIB_PATH
