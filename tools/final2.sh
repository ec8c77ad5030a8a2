# round 6: the whole GPU suite, smoke and the C2 / C4 lines on the final build
export TMPDIR=/tmp
out=gpurun_out/final2; mkdir -p $out; st=$out/status.txt
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $out/pytest.log 2>&1
rc=$?; echo "tests rc=$rc $(tail -1 $out/pytest.log)" >> $st
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $out/smoke.txt 2>&1
rc=$?; echo "smoke rc=$rc $(tail -1 $out/smoke.txt)" >> $st
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full > $out/bench_c2.log 2>&1
rc=$?; echo "c2 rc=$rc $(python tools/show.py $out/bench_c2.log 2>/dev/null | head -1)" >> $st
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --fit align --nsub 1000 --nchan 256 --nbin 1024 --steps 50 --warmup 5 > $out/bench_c4.log 2>&1
rc=$?; echo "c4 rc=$rc $(python tools/show.py $out/bench_c4.log 2>/dev/null | head -1)" >> $st
echo end >> $st
