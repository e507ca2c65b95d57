// tests/node/run_batch.mjs — TEST INFRASTRUCTURE: the type-erased ts/simulateTRANBatch.ts under Node 12 against libspicey_hip.so.
//   node --harmony-nullish --harmony-optional-chaining run_batch.mjs <erased_dir> <circuits.json> <out.json> [exact]
// circuits.json: a list of circuits as run_dropin.mjs reads one.
import fs from "fs"
import path from "path"
import { pathToFileURL } from "url"

const [, , erased, cktPath, outPath, mode] = process.argv
const main = async () => {
  const out = {}
  try {
    const { simulateTRANBatch } = await import(pathToFileURL(path.join(erased, "simulateTRANBatch.mjs")).href)
    const ckts = JSON.parse(fs.readFileSync(cktPath, "utf8")).map((j) => ({
      nodes: { rev: j.nodes, count: () => j.nodes.length },
      R: j.R, C: j.C, L: j.L, S: j.S, D: j.D,
      V: j.V.map((v) => ({ ...v, waveform: v.table ? (t) => v.table[Math.round(t / j.dt)] : null })),
      analyses: j.analyses, probes: j.probes,
    }))
    const enc = (x) => (Number.isFinite(x) ? x : String(x))
    const res = simulateTRANBatch(ckts, { exactOrder: mode === "exact" })
    out.slots = res.map((r, i) => {
      if (r === null) return null
      if (r instanceof Error) return { error: r.message }
      const ckt = ckts[i]
      const s = { times: r.times, keysV: Object.keys(r.nodeVoltages), keysI: Object.keys(r.elementCurrents), V: {}, I: {}, skipRisk: r.skipRisk,
                  state: { vPrev: ckt.C.map((c) => c.vPrev), iPrev: ckt.L.map((l) => l.iPrev), vdPrev: ckt.D.map((d) => d.vdPrev), isOn: ckt.S.map((x) => x.isOn) } }
      for (const k of s.keysV) s.V[k] = r.nodeVoltages[k].map(enc)
      for (const k of s.keysI) s.I[k] = r.elementCurrents[k].map(enc)
      return s
    })
  } catch (e) {
    out.error = String(e && e.message ? e.message : e)
  }
  fs.writeFileSync(outPath, JSON.stringify(out))
}
main()
