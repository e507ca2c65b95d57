# usage: bash tools/ab_ac_libs.sh libA.so libB.so  — same-session A/B of two builds of libspicey_hip.so on the plain AC sweep (tools/ac_probe.py)
for rep in 1 2 3; do for lib in "$@"; do echo "LIB $lib"; SPICEY_HIP_LIB=$lib timeout -k 10 100 python tools/ac_probe.py --n 1000 --inst 1 64 --check 0 || exit 1; done; done
for rep in 1 2 3; do for lib in "$@"; do echo "LIB $lib"; SPICEY_HIP_LIB=$lib timeout -k 10 100 python tools/ac_probe.py --n 200 --inst 8 64 --check 0 --no-resident || exit 1; done; done
