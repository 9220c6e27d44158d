for k in 1 2 4 1 2 4; do
  out=$(timeout -k 10 120 python3 bench.py --full --no-cpu --sustain 0 --steps 30 --ingest-steps 100 --ingest-streams $k 2>/dev/null) || exit $?
  echo "$out" | python3 -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); i=d['ingest']; print('streams', $k, i['frames_per_s'], i['h2d_GBs_per_gpu'], i['bit_exact'], d['value'])"
done
