#!/bin/bash
# The one GPU-box runner (via gpurun): named steps, in the order given, each under its own time limit,
# stdout / stderr of step <name> in gpurun_out/<name>_<TAG>.out / .err.  The script stops at the first failing step, so nothing touches the GPU
# after a timeout, abort or fault.
#
#   tools/gpu_run.sh smoke tests bench            # the round trip
#   TAG=r06 tools/gpu_run.sh bench kprof profile  # round evidence (then: python tools/pmc_summary.py r06)
#   AB="ab/base.so ab/new.so" tools/gpu_run.sh ab # in-process A/B of two builds (tools/build_variant.sh)
#
# Steps (environment knobs in brackets):
#   smoke      __graft_entry__.smoke()
#   tests      pytest -m gpu, one process, per-test limits                       [PYTEST_ARGS]
#   bench      the bench line with every side measurement (bench.py --full)      [BENCH_ARGS]
#   kprof      instrumented counts of one 100-spp config-4 frame, wave- and lane-level per region
#              (tools/kprofile.py; then here: python tools/region_table.py <kprof.json>)  [KPROF_ARGS]
#   profile    rocprofv3 kernel trace + separate PMC passes (tools/profile.sh)
#   ab         tools/ab_libs.py on config 4's whole frame (ring mode) and rank 0 of 8 (direct)  [AB SPP ROUNDS]
#   ab_ch9     the same on chapter 9 (config 2)                                  [AB ROUNDS]
#   pmc_ab     PMC passes over an in-process A/B (tools/pmc_ab.sh)               [AB ARGS]
#   ranksim    every rank's rows in bench.py's N > 1 frame pipeline (tools/rank_sim.py)  [NS PIPE RANKSIM_ARGS]
#   configs    every BASELINE config (tools/configs_bench.py)
#   dropin     the drop-in's one-shot cost per fresh process (tools/dropin_cold.py)  [DROPIN_CONFIGS]
#   progressive  config 4 accumulated in 1 / 10 / 50 passes with a resolve after each: wall time and the
#              per-pass overhead (tools/progressive_cost.py; its JSON on stdout is kept as
#              profiles/progressive/cost.json)
#   adaptive   what adaptive sampling costs on config 4: gather passes against row passes, sparse lists,
#              select / resolve, one render_adaptive run (tools/adaptive_cost.py; its JSON on stdout is
#              kept as profiles/adaptive/cost.json).  Its GPU tests (tests/test_gpu_adaptive.py) run
#              with the `tests` step
#   features   what a feature pass costs: rt_render_rows_features at 16 samples against a bounce_max = 1
#              colour pass on the same rays, on config 4's image and the 400x225 chapter-13 image
#              (tools/feature_cost.py; its JSON on stdout is kept as profiles/features/cost.json).  Its
#              GPU tests (tests/test_gpu_features.py) run with the `tests` step
#   trace      what a ray query costs: rt_trace_rays on 15.36 M coherent camera rays against the feature
#              pass at 16 samples plus a copy of the bytes it moves, and the incoherent, far-origin and
#              tiny-batch figures (tools/trace_cost.py; its JSON on stdout is kept as
#              profiles/trace/cost.json).  Its GPU tests (tests/test_gpu_trace.py) run with the `tests` step
#   occlusion  what an occlusion query costs against the closest-hit query on the same rays: primary
#              visibility, shadow rays and segments to a point light (tools/occlusion_cost.py; its JSON on
#              stdout is kept as profiles/occlusion/cost.json).  Its GPU tests (tests/test_gpu_occlusion.py)
#              run with the `tests` step
#   radiance   what a radiance query costs against the renderer on the same paths: rt_radiance_rays at 16
#              samples of 960,000 pixel-centre rays against rt_render_rows_accumulate, the one-sample,
#              permuted and tiny-batch figures (tools/radiance_cost.py; its JSON on stdout is kept as
#              profiles/radiance/cost.json).  Its GPU tests (tests/test_gpu_radiance.py) run with the
#              `tests` step
#   denoise   what rt_denoise costs against the 16-sample gather pass it stands in for, per level and
#              kernel form, and the RMSE table against a 500-spp frame, on config 4's image
#              (tools/denoise_cost.py; the "cost" and "quality" objects of its JSON on stdout are kept
#              as profiles/denoise/cost.json and quality.json).  Its GPU
#              tests (tests/test_gpu_denoise.py) run with the `tests` step
#   temporal  what rt_temporal_accumulate costs against rt_denoise at its default levels on config 4's
#              image, and the RMSE per frame of a 12-frame camera path with the temporal pass off and on
#              (tools/temporal_cost.py; the "cost" and "quality" objects of its JSON on stdout are kept
#              as profiles/temporal/cost.json and quality.json).  Its GPU tests
#              (tests/test_gpu_temporal.py) run with the `tests` step
#   peak      event-timed VALU peak and issue-cost table (tools/bin/peak_rates, built beforehand)
#   diag       bounds-checked builds through tools/diag_modes.py (ab/bounds*.so)
#   uselib     copy $LIB (an ab/*.so build) over the in-tree librtzig.so for the steps after it (on the
#              box's copy of the tree only)                                     [LIB]
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd "$(dirname "$0")/.."
mkdir -p gpurun_out
export TMPDIR=/tmp
T=${TAG:-run}
AB=${AB:-"ab/base.so ab/new.so"}

run() {  # run <name> <seconds> <command...>: stdout to gpurun_out/<name>_<tag>.out, stderr to .err;
         # stop on failure
  local name=$1 secs=$2; shift 2
  timeout -k 10 "$secs" "$@" > "gpurun_out/${name}_$T.out" 2> "gpurun_out/${name}_$T.err"
  local rc=$?
  echo "== $name rc=$rc"; tail -c 1500 "gpurun_out/${name}_$T.out"; echo; tail -3 "gpurun_out/${name}_$T.err"
  [ $rc -eq 0 ] || exit $rc
}

for step in "$@"; do
  case $step in
    smoke)   run smoke 200 python3 -u -c "import __graft_entry__ as g; g.smoke()" ;;
    tests)   run gputest 900 python3 -u -m pytest tests -m gpu -x -v --timeout 150 --timeout-method thread $PYTEST_ARGS ;;
    bench)   run bench 300 python3 -u bench.py --full $BENCH_ARGS ;;
    kprof)   run kprof 200 python3 -u tools/kprofile.py --spp 100 --variants bvh --out "gpurun_out/kprof_$T.json" $KPROF_ARGS ;;
    profile) TAG=$T bash tools/profile.sh || exit $? ;;
    ab)      run ab_full 300 python3 -u tools/ab_libs.py $AB --spp ${SPP:-100} --rounds ${ROUNDS:-7}
             run ab_r8 300 python3 -u tools/ab_libs.py $AB --spp 500 --row-step 8 --rounds ${ROUNDS:-7} ;;
    ab_ch9)  run ab_ch9 200 python3 -u tools/ab_libs.py $AB --scene ch9 --width 400 --aspect 1.7777777777777777 --spp 100 --rounds ${ROUNDS:-9} ;;
    pmc_ab)  TAG=$T AB="$AB" bash tools/pmc_ab.sh || exit $? ;;
    ranksim) run ranksim 300 python3 -u tools/rank_sim.py --ns ${NS:-1 2 4 8} --reps 2 --pipe-frames 8 --pipe-mode ${PIPE:-deferred} $RANKSIM_ARGS ;;
    configs) run configs 300 python3 -u tools/configs_bench.py --out "gpurun_out/configs_$T.json" ;;
    dropin)  run dropin 300 python3 -u tools/dropin_cold.py --runs 3 --configs ${DROPIN_CONFIGS:-2,4,5} ;;
    progressive) run progressive 200 python3 -u tools/progressive_cost.py ;;
    adaptive) run adaptive 300 python3 -u tools/adaptive_cost.py ;;
    features) run features 200 python3 -u tools/feature_cost.py ;;
    trace)   run trace 300 python3 -u tools/trace_cost.py ;;
    occlusion) run occlusion 300 python3 -u tools/occlusion_cost.py ;;
    radiance) run radiance 300 python3 -u tools/radiance_cost.py ;;
    denoise) run denoise 300 python3 -u tools/denoise_cost.py ;;
    temporal) run temporal 300 python3 -u tools/temporal_cost.py ;;
    peak)    run peak 300 ./tools/bin/peak_rates ${PEAK_MS:-60} ${PEAK_MODE:-2} ;;
    diag)    run diag 300 python3 -u tools/diag_modes.py raytracing-with-zig_amd/librtzig.so ab/bounds.so --oracle-row ;;
    uselib)  cp "$LIB" raytracing-with-zig_amd/librtzig.so || exit 2; echo "== using $LIB" ;;
    *) echo "unknown step: $step"; exit 2 ;;
  esac
done
exit 0
