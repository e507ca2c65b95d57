// ts/simulate.ts — the public entry (reference: lib/analysis/simulate.ts:5-10): parse, AC sweep if the netlist has an .ac
// card, transient if it has a .tran card.  Both analyses run natively (ts/spiceyHip.ts -> libspicey_hip.so).
import { parseNetlist } from "./parseNetlist"
import { simulateAC } from "./simulateAC"
import { simulateTRAN } from "./simulateTRAN"

export type SimulateOptions = {
  /** the transient runs the reference-order engine (simulateTRAN); the AC sweep is unaffected */
  exactOrder?: boolean
  /** the AC sweep runs the reference-order AC engine (simulateAC); the transient is unaffected */
  acExactOrder?: boolean
}

export function simulate(netlistText: string, options?: SimulateOptions) {
  const circuit = parseNetlist(netlistText)
  const ac = simulateAC(circuit, { exactOrder: !!options?.acExactOrder })
  const tran = simulateTRAN(circuit, { exactOrder: !!options?.exactOrder })
  return { circuit, ac, tran }
}
