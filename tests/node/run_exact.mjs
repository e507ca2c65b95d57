// tests/node/run_exact.mjs — TEST INFRASTRUCTURE: the type-erased ts/simulateTRAN.ts with { exactOrder: true } under Node 12
// against libspicey_hip.so (the reference-order engine).
//   node --harmony-nullish --harmony-optional-chaining run_exact.mjs <erased_dir> <circuit.json> <out.json>
// circuit.json as for run_dropin.mjs.
import fs from "fs"
import path from "path"
import { pathToFileURL } from "url"

const [, , erased, cktPath, outPath] = process.argv
const main = async () => {
  const out = {}
  try {
    const { simulateTRAN } = await import(pathToFileURL(path.join(erased, "simulateTRAN.mjs")).href)
    const j = JSON.parse(fs.readFileSync(cktPath, "utf8"))
    const ckt = {
      nodes: { rev: j.nodes, count: () => j.nodes.length },
      R: j.R, C: j.C, L: j.L, S: j.S, D: j.D,
      V: j.V.map((v) => ({ ...v, waveform: v.table ? (t) => v.table[Math.round(t / j.dt)] : null })),
      analyses: j.analyses, probes: j.probes,
    }
    const r = simulateTRAN(ckt, { exactOrder: true })
    const enc = (x) => (Number.isFinite(x) ? x : String(x))
    out.tran = { times: r.times, keysV: Object.keys(r.nodeVoltages), keysI: Object.keys(r.elementCurrents), V: r.nodeVoltages, I: {}, skipRisk: r.skipRisk,
                 state: { vPrev: ckt.C.map((c) => c.vPrev), iPrev: ckt.L.map((l) => l.iPrev), vdPrev: ckt.D.map((d) => d.vdPrev), isOn: ckt.S.map((s) => s.isOn) } }
    for (const k of out.tran.keysI) out.tran.I[k] = r.elementCurrents[k].map(enc)
  } catch (e) {
    out.error = String(e && e.message ? e.message : e)
  }
  fs.writeFileSync(outPath, JSON.stringify(out))
}
main()
