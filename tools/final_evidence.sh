ROOT=$(cd "$(dirname "$0")/.." && pwd)   # the repository root
# The evidence of a round from ONE machine with an MI355X, into $O (default out/): smoke, the full GPU test run on the
# default flavour, the --full bench line with the rocprofv3 summaries / timeline / PMC traffic (tools/refresh_profiles.sh),
# the distributed lines (tools/dist_lines.sh).
#   O=<output directory> bash tools/final_evidence.sh
cd $ROOT
O=${O:-out}; mkdir -p $O; O=$(cd $O && pwd)
R=${R:-r06}
python -c "import __graft_entry__ as g; g.smoke()" > $O/${R}_smoke.log 2>&1; tail -1 $O/${R}_smoke.log
timeout -k 10 700 python -m pytest tests -m gpu -q > $O/${R}_gputests_default.log 2>&1; tail -2 $O/${R}_gputests_default.log
R=$R O=$O bash tools/refresh_profiles.sh > $O/${R}_refresh.log 2>&1; tail -c 300 $O/${R}_bench_default.json; echo
R=$R O=$O bash tools/dist_lines.sh > $O/${R}_dist_lines.log 2>&1; tail -c 200 $O/${R}_bench_rccl1.json; echo
