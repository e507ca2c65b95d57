// tests/node/run_ac_exact.mjs — TEST INFRASTRUCTURE: the type-erased ts/simulateAC.ts with { exactOrder: true } under Node 12
// against libspicey_hip.so (the reference-order AC engine).
//   node --harmony-nullish --harmony-optional-chaining run_ac_exact.mjs <erased_dir> <circuit.json> <out.json>
// circuit.json as for run_dropin.mjs.  Complex values are written as [re, im].
import fs from "fs"
import path from "path"
import { pathToFileURL } from "url"

const [, , erased, cktPath, outPath] = process.argv
const main = async () => {
  const out = {}
  try {
    const { simulateAC } = await import(pathToFileURL(path.join(erased, "simulateAC.mjs")).href)
    const j = JSON.parse(fs.readFileSync(cktPath, "utf8"))
    const ckt = {
      nodes: { rev: j.nodes, count: () => j.nodes.length },
      R: j.R, C: j.C, L: j.L, S: j.S, D: j.D, V: j.V,
      analyses: j.analyses, probes: j.probes,
    }
    const r = simulateAC(ckt, { exactOrder: true })
    const pack = (rec) => { const o = {}; for (const k of Object.keys(rec)) o[k] = rec[k].map((z) => [z.re, z.im]); return o }
    out.ac = { freqs: r.freqs, keysV: Object.keys(r.nodeVoltages), keysI: Object.keys(r.elementCurrents), V: pack(r.nodeVoltages), I: pack(r.elementCurrents) }
  } catch (e) {
    out.error = String(e && e.message ? e.message : e)
  }
  fs.writeFileSync(outPath, JSON.stringify(out))
}
main()
